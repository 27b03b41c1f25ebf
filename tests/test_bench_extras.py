"""Which of bench.py's untimed extras a run does: none on a plain run, the rest only with --full."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

ALL = {"e2e", "e2e_at_scale", "host_path", "post", "bins", "config2", "cpu_baseline"}


def test_plain_run_does_no_extra():
    args = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not args.full
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        assert bench.extras_to_run(args, rank, world) == frozenset()
    args = bench.parse_args(["--dump-outputs", "out"])
    assert bench.extras_to_run(args, 0, 1) == frozenset()


def test_full_run_does_every_extra_its_switches_leave_on():
    assert bench.extras_to_run(bench.parse_args(["--full"]), 0, 1) == ALL
    off = bench.parse_args(["--full", "--no-pcie", "--no-bins", "--no-post", "--cpu-seconds", "0"])
    assert bench.extras_to_run(off, 0, 1) == {"e2e", "e2e_at_scale", "config2"}
    assert bench.extras_to_run(bench.parse_args(["--full", "--e2e-bases", "0"]), 0, 1) == ALL - {"e2e_at_scale"}
    assert bench.extras_to_run(bench.parse_args(["--full", "--no-e2e", "--no-config2"]), 0, 1) == ALL - {"e2e", "e2e_at_scale", "config2"}


def test_full_run_with_several_ranks():
    args = bench.parse_args(["--gpus", "2", "--full"])
    assert bench.extras_to_run(args, 0, 2) == {"host_path", "post"}
    assert bench.extras_to_run(args, 1, 2) == {"host_path"}
