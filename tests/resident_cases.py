"""Cases for the mapper's resident path (seeding_on_device = 2) outside the read-overlap presets: map-ont / map-pb with --no-long-join and map-ont -r 500,500, where
mm_set_parent / mm_select_sub drop records and a kept record's divergence has to come from the place it had among all chains.  The chimeric read set and the runs
recorded from the reference program (tests/golden/resident, made by tests/tools/gen_golden_resident.py), and how this project's mapper is called on them.
Test infrastructure only: imported by tests/test_resident_cpu.py, tests/test_gpu_resident.py and tests/tools/gen_golden_resident.py."""
import hashlib
import json
import os
import tempfile

import numpy as np

import golden_io
import mm2gb_amd as mm
import sim_reads
from test_seeding_cpu import read_fasta

GOLD = os.path.join(golden_io.GOLD, "resident")
INF = 2**31 - 1
SKIPS = {"s25": 25, "inf": INF}
ONT, PB = dict(k=15, w=10, hpc=False), dict(k=19, w=10, hpc=True)
# kind: (the reference program's arguments, the index parameters, this project's option fields).  map-pb's mapping options are map-ont's (options.c:102-103).
KINDS = {
    "map-ont": (["-x", "map-ont", "--no-long-join"], ONT, dict(flag=mm.F_NO_LJOIN)),
    "map-pb": (["-x", "map-pb", "--no-long-join"], PB, dict(flag=mm.F_NO_LJOIN)),
    "r500": (["-x", "map-ont", "-r", "500,500"], ONT, dict(bw=500, bw_long=500)),      # bw_long <= bw without MM_F_NO_LJOIN: the other way into the resident path
}
RUNS = ["chim.map-ont", "chim.map-pb", "chim.r500", "sim160.map-ont", "sim160.map-pb"]
CHIM_SEED = 7
MIN_MOVED, MIN_TP_S = 10, 10          # what the generator asserts and tests/test_resident_cpu.py checks again


# ---------------------------------------------------------------- the chimeric set
def chim_genome(rng):
    """120 kb: 20 000-28 000 copied to 70 000-78 000 at 12 % divergence (secondary chains that mm_select_sub drops or keeps), and a 40-unit tandem array of a
    90-base unit at 100 000 (many short chains inside one read)."""
    g = sim_reads.BASES[rng.integers(0, 4, 120_000)].copy()
    g[70_000:78_000] = sim_reads.mutate(rng, g[20_000:28_800], 0.12)[:8_000]
    g[100_000:103_600] = np.tile(sim_reads.BASES[rng.integers(0, 4, 90)], 40)
    return g


def sim_chim(seed=CHIM_SEED):
    """(genome bytes, [(name, bytes)]): 60 reads at 4-9 % error on a random strand, of three kinds in turn -- 5-7 kb from the copied region followed by 1-2 kb from
    elsewhere (either strand), 5-8 kb through the tandem array followed by 0.8-2 kb from elsewhere, a plain 2-8 kb read -- and one that is not from the genome."""
    rng = np.random.default_rng(seed)
    g = chim_genome(rng)
    piece = lambda st, n, err: sim_reads.mutate(rng, g[st:st + n], err)
    reads = []
    for r in range(60):
        err = float(rng.uniform(0.04, 0.09))
        if r % 3 == 0:
            s = piece(int(rng.integers(20_000, 21_000)), int(rng.integers(5_000, 7_000)), err)
            t = piece(int(rng.integers(40_000, 60_000)), int(rng.integers(1_000, 2_000)), err)
            s = np.concatenate([s, sim_reads.revcomp(t) if rng.random() < 0.5 else t])
        elif r % 3 == 1:
            s = piece(int(rng.integers(97_000, 99_500)), int(rng.integers(5_000, 8_000)), err)
            s = np.concatenate([s, piece(int(rng.integers(5_000, 15_000)), int(rng.integers(800, 2_000)), err)])
        else:
            n = int(rng.integers(2_000, 8_000))
            s = piece(int(rng.integers(0, len(g) - n)), n, err)
        reads.append((f"chim{r}", (sim_reads.revcomp(s) if rng.random() < 0.5 else s).tobytes()))
    reads.append(("stray", sim_reads.BASES[rng.integers(0, 4, 3_000)].tobytes()))
    return g.tobytes(), reads


_sim160 = None


def sim160():
    """([(name, bytes)] references, [(name, bytes)] reads) of tests/golden/sim160.json, regenerated from its seed and checked against its md5s; the reference program
    gives every one of the 160 reads a line, so one read that is not from the genome follows them (a set has to hold a read without a line)."""
    global _sim160
    if _sim160 is None:
        meta = json.load(open(os.path.join(golden_io.GOLD, "sim160.json")))
        with tempfile.TemporaryDirectory() as d:
            ref, reads = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")
            sim_reads.simulate(ref, reads, seed=meta["seed"], n_reads=meta["n_reads"], len_lo=meta["len_lo"], len_hi=meta["len_hi"], tandem=meta["tandem"])
            assert hashlib.md5(open(ref, "rb").read()).hexdigest() == meta["ref_md5"], "simulator drifted: regenerate the golden"
            assert hashlib.md5(open(reads, "rb").read()).hexdigest() == meta["reads_md5"]
            stray = sim_reads.BASES[np.random.default_rng(meta["seed"] + 1_000).integers(0, 4, 3_000)].tobytes()
            _sim160 = (read_fasta(ref), read_fasta(reads) + [("stray", stray)])
    return _sim160


# ---------------------------------------------------------------- the fixture
_gold = None


def gold():
    """The committed fixture (resident.npz: one JSON document, compressed): {"seed", "ref": [[name, sequence]], "reads": [[name, sequence]] (the chimeric set),
    "paf": {"<run>.<skip>": text}, "moved": {"<chim run>.<skip>": reads with a kept record at a moved place and another dv there}, "tp_S": {"<sim160 run>.<skip>": lines}}."""
    global _gold
    if _gold is None:
        _gold = json.loads(np.load(os.path.join(GOLD, "resident.npz"))["doc"].tobytes().decode("utf-8"))
    return _gold


def refs_of(name):
    return sim160()[0] if name == "sim160" else [(n, s.encode()) for n, s in gold()["ref"]]


def reads_of(name):
    return sim160()[1] if name == "sim160" else [(n, s.encode()) for n, s in gold()["reads"]]


def golden_paf(run, skip):
    return gold()["paf"][f"{run}.{skip}"]


def lines_of(paf, names):
    """The lines of `paf` whose query is one of `names`, in the order of the text."""
    names = set(names)
    return "".join(ln + "\n" for ln in paf.splitlines() if ln.split("\t")[0] in names)


def dv_of(fields):
    return next(t for t in fields[12:] if t.startswith("dv:f:"))


def moved_reads(kept, all_chains):
    """Reads of a run that keep a record whose place among the read's kept records differs from its place among all the read's chains (the same run with -P) while
    the chain at the kept place has another dv:f: -- a divergence looked up by the kept place would show.  Records are identified by the first nine PAF columns."""
    by_read = lambda text: {q: [f for f in (ln.split("\t") for ln in text.splitlines()) if f[0] == q] for q in dict.fromkeys(ln.split("\t")[0] for ln in text.splitlines())}
    k, p = by_read(kept), by_read(all_chains)
    out = []
    for q, recs in k.items():
        keys = [tuple(f[:9]) for f in p.get(q, [])]
        for at, f in enumerate(recs):
            was = keys.index(tuple(f[:9])) if tuple(f[:9]) in keys else -1
            if was >= 0 and was != at and dv_of(p[q][at]) != dv_of(p[q][was]):
                out.append(q)
                break
    return out


# ---------------------------------------------------------------- this project's mapper on them
_index = {}


def index_for(run):
    """The SeedIndex of a run's references, kept for the process (host-built): one per read set and index parameters."""
    name, kind = run.split(".")
    kw = KINDS[kind][1]
    key = (name, kw["k"], kw["hpc"])
    if key not in _index:
        _index[key] = mm.SeedIndex([s for _, s in refs_of(name)], threads=4, **kw)
    return _index[key]


def options(run, skip="inf", **fields):
    _, kw, own = KINDS[run.split(".")[1]]
    return mm.map_opt(**{**own, "max_chain_skip": SKIPS[skip], "host_threads": 4, **fields}), kw["k"]


def map_run(engine, run, skip="inf", reads=None, **fields):
    """map_reads of a run (or of `reads` against the run's references) -> (PAF, stats)."""
    name = run.split(".")[0]
    opt, k = options(run, skip, **fields)
    return mm.map_reads(engine, index_for(run), [n for n, _ in refs_of(name)], reads_of(name) if reads is None else reads, opt=opt, k=k)


# ---------------------------------------------------------------- batches made for the fall-backs and the early returns
ODD = [("empty", b""), ("short", b"ACGTACGTAC"), ("n_only", b"N" * 500)]      # the reads of tests/test_gpu_mapper.py that cannot have a minimizer
PIECE_SEED, NO_HIT_SEED = 21, 22


def host_hits(run, seq):
    """The hits the host's seeding finds for one read against a run's index (what the device's seeding counts per batch)."""
    ix = index_for(run)
    return len(ix.matches(seq, ix.mid_occ())["hits"]) if len(seq) else 0


def no_hit_reads(run, n, length=3_000, seed=NO_HIT_SEED):
    """n random reads that share no selected minimizer with the run's references (checked on the host: a random read meets a 15-mer of 120 kb now and then)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        s = sim_reads.BASES[rng.integers(0, 4, length)].tobytes()
        if host_hits(run, s) == 0:
            out.append((f"random{len(out)}", s))
    return out


def piece_reads(run="chim.map-ont", n=12, seed=PIECE_SEED):
    """Random 2 kb reads that each hold one exact piece of 30-60 bases of the chimeric genome (from its unique part) and have a hit, but nothing that chains: a
    chain's score is at most the bases its anchors cover, so a piece below min_chain_score = 40 bases cannot chain, and of the longer pieces those are kept that
    give fewer hits than min_cnt = 3 (counted on the host)."""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(gold()["ref"][0][1].encode(), dtype=np.uint8)
    out = []
    while len(out) < n:
        s = sim_reads.BASES[rng.integers(0, 4, 2_000)].copy()
        at, st, ln = int(rng.integers(100, 1_800)), int(rng.integers(30_000, 60_000)), int(rng.integers(30, 61))
        s[at:at + ln] = g[st:st + ln]
        hits = host_hits(run, s.tobytes())
        if hits >= 1 and (ln < 40 or hits < 3):
            out.append((f"piece{len(out)}_{ln}", s.tobytes()))
    return out


def stream_chunks(lens, chunk_bases):
    """mm2gb_map_reads_stream's cuts: [(first read, one past the last)]."""
    cut, acc = [0], 0
    for r, n in enumerate(lens):
        acc += n
        if acc >= chunk_bases and r + 1 < len(lens):
            cut.append(r + 1)
            acc = 0
    cut.append(len(lens))
    return list(zip(cut[:-1], cut[1:]))
