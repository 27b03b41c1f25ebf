"""The chaining DP with mg_lchain_dp's skip limit kept (lchain.c:183-187): the engine's opt-in mode (Engine(chain_skip=True),
mm2gb_engine_set_chain_skip, MM2GB_CHAIN_SKIP=keep) against the reference's vectors recorded at finite limits, the CPU oracle under
random limits, and the reference's CPU program at minimap2's default max_chain_skip (25) and at 0.  The default mode stays exhaustive."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_io
import orc
import synth_cases as sc

pytestmark = pytest.mark.gpu

mm = pytest.importorskip("mm2gb_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = golden_io.GOLD
REF = os.path.join(ROOT, "oracle", "_ref")
CFG = os.path.join(ROOT, "mm2-gb_amd", "mi355x_config.json")
PAIRS = {"mt": ("MT-human.fa", "MT-orang.fa"), "inv": ("t-inv.fa", "q-inv.fa"), "q2": ("t2.fa", "q2.fa")}
FINITE = [p for p in golden_io.all_cases() if golden_io.load(p)["prm"].max_skip != orc.INT32_MAX]


def misc_from(prm):
    return mm.default_misc(max_iter=prm.max_iter, max_dist_x=prm.max_dist_x, max_dist_y=prm.max_dist_y, max_skip=prm.max_skip,
                           bw=prm.bw, min_cnt=prm.min_cnt, min_score=prm.min_sc, is_cdna=prm.is_cdna, n_seg=prm.n_seg,
                           chn_pen_gap=np.float32(prm.pen_gap), chn_pen_skip=np.float32(prm.pen_skip))


def rel(p):
    idx = np.arange(len(p), dtype=np.int64)
    return np.where(p >= 0, idx - p, 0).astype(np.int32)


def rel_many(po, off):
    return np.concatenate([rel(po[off[r]:off[r + 1]]) for r in range(len(off) - 1)]) if off[-1] else np.zeros(0, np.int32)


def cpu_threads():
    import bench
    return max(1, bench.cpu_quota())


@pytest.fixture(scope="module")
def engine():
    with mm.Engine(chain_skip=True) as e:
        yield e


def check_against_oracle(engine, a, off, prm):
    engine.set_misc(misc_from(prm))
    f, p, st = engine.score(a, off)
    fo, po, pairs = orc.chain_fill_many(a, off, prm, threads=cpu_threads())
    po_rel = rel_many(po, off)
    bad = np.flatnonzero((f != fo) | (p != po_rel))
    assert bad.size == 0, (f"max_skip {prm.max_skip} max_iter {prm.max_iter}: {bad.size} anchors differ, first at {bad[:5]}: "
                           f"gpu f/p {f[bad[:5]]}/{p[bad[:5]]} oracle {fo[bad[:5]]}/{po_rel[bad[:5]]}")
    assert st["n_pairs"] == pairs                       # the sum of window sizes, whatever the walks met
    assert engine.last_score_form() == (1 if prm.max_skip < prm.max_iter else 0)
    return f, p


def test_modes_are_per_engine():
    with mm.Engine() as e:
        assert e.last_score_form() == 0
        e.set_chain_skip(True)
        e.set_chain_skip(False)
    with pytest.raises(mm.Mm2gbError):
        mm._check(mm.lib().mm2gb_engine_set_chain_skip(None, 1))


@pytest.mark.parametrize("path", FINITE, ids=golden_io.case_ids(FINITE))
def test_reference_vectors_at_their_finite_limit(engine, path):
    """Every committed vector recorded at a finite max_skip: f / p, then chains and compacted anchors through the device post-pass
    and the host post-pass, all equal to what the reference recorded."""
    g = golden_io.load(path)
    prm, a = g["prm"], g["a"]
    off = np.array([0, len(a)], dtype=np.int64)
    engine.set_misc(misc_from(prm))
    f, p, _ = engine.score(a, off)
    assert engine.last_score_form() == 1
    assert np.array_equal(f, g["f"]) and np.array_equal(p, rel(g["p"]))
    for res, _ in (engine.chain(a, off, threads=2), engine.chain_gpu(a, off)):
        assert np.array_equal(res[0][0], g["u"]) and np.array_equal(res[0][1], g["a_out"])
    # and the exhaustive default still gives the infinite-limit answer on the same misc
    with mm.Engine(misc=misc_from(prm)) as e:
        f2, p2, _ = e.score(a, off)
        assert e.last_score_form() == 0
        prm.max_skip = orc.INT32_MAX
        fo, po, _ = orc.chain_fill(a, prm)
        assert np.array_equal(f2, fo) and np.array_equal(p2, rel(po))


_LCHAIN_DP = r"""
import ctypes as C, json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import golden_io, mm2gb_amd as mm
L, libc = mm.lib(), C.CDLL(None)
libc.malloc.restype = C.c_void_p; libc.malloc.argtypes = [C.c_size_t]; libc.free.argtypes = [C.c_void_p]
bad = []
for path in sys.argv[2:]:
    g = golden_io.load(path); a = np.ascontiguousarray(g["a"]); prm = g["prm"]
    buf = libc.malloc(a.nbytes); C.memmove(buf, a.ctypes.data, a.nbytes)
    n_u, u_ptr = C.c_int(0), C.c_void_p(0)
    out = L.mm2gb_lchain_dp(prm.max_dist_x, prm.max_dist_y, prm.bw, prm.max_skip, prm.max_iter, prm.min_cnt, prm.min_sc,
                            prm.pen_gap, prm.pen_skip, prm.is_cdna, prm.n_seg, len(a), buf, C.byref(n_u), C.byref(u_ptr), None)
    u = np.ctypeslib.as_array(C.cast(u_ptr, C.POINTER(C.c_uint64)), shape=(n_u.value,)).copy() if n_u.value else np.zeros(0, np.uint64)
    n_out = int((u & 0xffffffff).sum())
    a_out = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n_out, 2)).copy() if n_out else np.zeros((0, 2), np.uint64)
    if not (np.array_equal(u, g["u"]) and np.array_equal(a_out, g["a_out"])): bad.append(g["name"])
    if u_ptr.value: libc.free(u_ptr)
    if out: libc.free(out)
print(json.dumps(bad))
"""


def test_lchain_dp_entry_keeps_the_limit_with_the_knob():
    """mm2gb_lchain_dp (mg_lchain_dp's signature, the drop-in's single-read entry) follows MM2GB_CHAIN_SKIP=keep, read when its engines
    are made: a fresh process with the knob set gives the reference's chains at every finite-limit vector."""
    env = dict(os.environ, MM2GB_CHAIN_SKIP="keep")
    r = subprocess.run([sys.executable, "-c", _LCHAIN_DP, ROOT, *FINITE], capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert json.loads(r.stdout.decode().strip().splitlines()[-1]) == []


def _mixed_batch(seed):
    """Reads of every shape the walk must get right: chains with indels, repeat blocks that fill max_iter, the max_ii rescue case,
    a grid of equal scores, varying spans, noise, and empty and one-anchor reads between them."""
    parts = [sc.colinear(3000, seed), sc.sort_by_x(np.concatenate([sc.repeat_block(6000, seed + 1), sc.colinear(800, seed + 2)])),
             np.zeros((0, 2), np.uint64), sc.rescue_case(n_noise=3000, seed=seed + 3), sc.noise(1, seed + 4), sc.grid_ties(),
             sc.variable_span(2000, seed + 5), np.zeros((0, 2), np.uint64), sc.read_like(20000, seed + 6), sc.noise(1, seed + 7)]
    off = np.cumsum([0] + [len(x) for x in parts]).astype(np.int64)
    return np.concatenate(parts).astype(np.uint64), off


@pytest.mark.parametrize("max_skip", [0, 1, 5, 25, 60, "max_iter-1"])
def test_oracle_under_random_limits(engine, max_skip):
    rng = np.random.default_rng(31 + (max_skip if isinstance(max_skip, int) else 99))
    a, off = _mixed_batch(int(rng.integers(1, 1000)))
    for max_iter in (orc.INT32_MAX, 5000, int(rng.integers(40, 400)), 64):
        ms = max_iter - 1 if max_skip == "max_iter-1" else max_skip
        check_against_oracle(engine, a, off, orc.default_param(max_skip=ms, max_iter=max_iter))


@pytest.mark.parametrize("max_skip", [0, 25])
def test_oracle_cdna_and_two_segments(engine, max_skip):
    a, off = _mixed_batch(77)
    check_against_oracle(engine, a, off, orc.default_param(max_skip=max_skip, is_cdna=1))
    parts = [sc.two_segments(4000, 5), sc.two_segments(2500, 6)]
    off2 = np.cumsum([0] + [len(x) for x in parts]).astype(np.int64)
    check_against_oracle(engine, np.concatenate(parts), off2, orc.default_param(max_skip=max_skip, n_seg=2))


@pytest.mark.timeout(900)
def test_long_reads_batch_every_anchor(engine):
    """100-300 kb reads (configs[3]'s shape), at least 20 M anchors, every anchor against the oracle at 25 and at 0."""
    import bench
    _, _, a, off = bench.shard_for_rank(mm, 0, 1, 2024, 20_000_000, 100_000, 300_000, threads=cpu_threads())
    assert len(a) >= 19_800_000
    for ms in (25, 0):
        check_against_oracle(engine, a, off, orc.default_param(max_skip=ms))


@pytest.mark.timeout(2400)
def test_bench_size_batch_at_25_every_anchor(engine):
    """BASELINE configs[3] at full size (500 M anchors of 100-300 kb reads) at minimap2's default limit: every anchor against the oracle.
    MM2GB_TEST_FULL_ANCHORS runs a smaller batch on a machine with less host memory."""
    import bench
    target = int(os.environ.get("MM2GB_TEST_FULL_ANCHORS", 500_000_000))
    _, _, a, off = bench.shard_for_rank(mm, 0, 1, 2024, target, 100_000, 300_000, threads=cpu_threads())
    prm = orc.default_param(max_skip=25)
    engine.set_misc(misc_from(prm))
    f, p, st = engine.score(a, off)
    assert engine.last_score_form() == 1 and st["n_anchors"] == len(a)
    fo, po, pairs = orc.chain_fill_many(a, off, prm, threads=cpu_threads())
    assert pairs == st["n_pairs"]
    assert np.array_equal(f, fo), f"{np.count_nonzero(f != fo)} scores differ"
    del fo
    for r in range(len(off) - 1):
        lo, hi = off[r], off[r + 1]
        assert np.array_equal(p[lo:hi], rel(po[lo:hi])), f"predecessors of read {r} differ"


def test_inert_limit_and_default_mode(engine):
    """max_skip >= max_iter cannot end a walk: the exhaustive kernel runs (form 0) and gives the same f / p.  An engine in the default
    mode ignores a finite max_skip."""
    a, off = _mixed_batch(5)
    for max_iter, ms in ((5000, 5000), (64, 64), (64, 1000)):
        f, p = check_against_oracle(engine, a, off, orc.default_param(max_skip=ms, max_iter=max_iter))
        assert engine.last_score_form() == 0
    with mm.Engine() as e:
        e.set_misc(misc_from(orc.default_param(max_skip=25)))
        f, p, _ = e.score(a, off)
        assert e.last_score_form() == 0
        fo, po, _ = orc.chain_fill_many(a, off, orc.default_param(), threads=4)
        assert np.array_equal(f, fo) and np.array_equal(p, rel_many(po, off))


@pytest.mark.timeout(300)
def test_unsorted_anchors_come_back(engine):
    """Broken input (not sorted by x) still returns; the read next to it is exact."""
    rng = np.random.default_rng(5)
    parts = [sc.sort_by_x(np.concatenate([sc.repeat_block(6000, 91), sc.colinear(500, 92)])), sc.read_like(8000, 93)]
    a = np.concatenate(parts)
    off = np.array([0, len(parts[0]), len(a)], np.int64)
    shuffled = a.copy()
    rng.shuffle(shuffled[: len(parts[0])])
    prm = orc.default_param(max_skip=25)
    engine.set_misc(misc_from(prm))
    f, p, st = engine.score(shuffled, off)
    assert engine.last_score_form() == 1 and len(f) == len(a)
    idx = np.arange(len(a))
    assert ((p >= 0) & (p <= idx - off[np.searchsorted(off, idx, side="right") - 1])).all()
    fo, po, _ = orc.chain_fill(parts[1], prm)
    assert np.array_equal(f[off[1]:], fo) and np.array_equal(p[off[1]:], rel(po))


# ---- reads in, PAF out at minimap2's default flags ----

def _read_fasta(path):
    from test_seeding_cpu import read_fasta
    return read_fasta(path)


def _map(ref_fa, reads_fa, **opt):
    refs, reads = _read_fasta(ref_fa), _read_fasta(reads_fa)
    with mm.Engine() as e, mm.SeedIndex([s for _, s in refs]) as ix:
        return mm.map_reads(e, ix, [n for n, _ in refs], reads, opt=mm.map_opt(**opt))


def _sim48(tmp_path):
    import sim_reads
    meta = json.load(open(os.path.join(GOLD, "sim160.json")))
    ref, reads = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    sim_reads.simulate(ref, reads, seed=meta["seed"], n_reads=48, len_lo=meta["len_lo"], len_hi=meta["len_hi"], tandem=meta["tandem"])
    return ref, reads


def _cpu_paf(ref, reads, skip):
    exe = os.path.join(REF, "minimap2_cpu")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/minimap2_cpu is missing (make -C oracle ref where the reference checkout exists)")
    r = subprocess.run([exe, "-t", "1", f"--max-chain-skip={skip}", ref, reads], capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode()


@pytest.mark.parametrize("case", sorted(PAIRS))
def test_own_host_reference_pairs_at_25(case):
    tgt, qry = PAIRS[case]
    paf, st = _map(os.path.join(GOLD, "data", tgt), os.path.join(GOLD, "data", qry), max_chain_skip=25)
    assert paf == open(os.path.join(GOLD, f"real_{case}_s25.paf")).read()


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("skip", [25, 0])
def test_own_host_simulated_reads_at_finite_limits(tmp_path, skip):
    ref, reads = _sim48(tmp_path)
    want = _cpu_paf(ref, reads, skip)
    paf, st = _map(ref, reads, max_chain_skip=skip)
    assert st["n_reads"] == 48
    if paf != want:
        g, w = paf.splitlines(), want.splitlines()
        bad = [k for k in range(min(len(g), len(w))) if g[k] != w[k]]
        raise AssertionError(f"{len(bad)} of {len(w)} PAF lines differ (got {len(g)}); first: {g[bad[0]] if bad else None} vs {w[bad[0]] if bad else None}")


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("host", ["minimap2_gpuhost", "minimap2_gpuhost_rmq"])
def test_drop_in_at_default_flags(tmp_path, host):
    """The reference's own host on this library with MM2GB_CHAIN_SKIP=keep, at no skip flag (minimap2's 25) and at 0: its PAF equals the
    reference CPU program's at the same flags, on the reference's test pairs and on simulated long reads."""
    exe = os.path.join(REF, host)
    if not os.path.exists(exe):
        pytest.fail(f"oracle/_ref/{host} is missing (make -C oracle gpuhost gpuhost_rmq where the reference checkout exists)")
    env = dict(os.environ, MM2GB_CHAIN_SKIP="keep")
    ref, reads = _sim48(tmp_path)
    inputs = [(os.path.join(GOLD, "data", t), os.path.join(GOLD, "data", q)) for t, q in PAIRS.values()] + [(ref, reads)]
    for flags, skip in (([], 25), (["--max-chain-skip=0"], 0)):
        for tgt, qry in inputs:
            r = subprocess.run([exe, "-t", "1", *flags, "--gpu-chain", "--gpu-cfg", CFG, tgt, qry], capture_output=True, timeout=900, env=env)
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            assert r.stdout.decode() == _cpu_paf(tgt, qry, skip), f"{host} {flags} {os.path.basename(qry)}"
