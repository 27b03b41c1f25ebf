for rep in 1 2; do
for t in ${TEAMS:-0 64 256 640 1500}; do
  MM2GB_POST_TEAM_READS=$t timeout 300 python bench.py --full --steps 1 --warmup 1 --cpu-seconds 0 --no-pcie --no-e2e --no-bins 2>/dev/null | tail -1 | python -c "
import json, sys; d=json.loads(sys.stdin.read()); print('team reads $t', 'post_pass_device ms', d['post_pass_device']['ms'])"
done
done
