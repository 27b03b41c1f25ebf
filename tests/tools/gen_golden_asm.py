"""Records tests/golden/asm and tests/golden/ksw/extd2_asm_cases.npz from the REFERENCE build (oracle/_ref), as data only.

options.json: for map-hifi, map-ccs, asm5, asm10 and asm20 what mm_set_opt(NULL) + mm_set_opt(name) leave in mm_mapopt_t / mm_idxopt_t (through
ctypes): every field of mm2gb_align_opt_t, the mapping fields of tests/asm_cases.MAP_FIELDS, and the index's k, w, hpc.

pafs.npz: what oracle/_ref/minimap2_cpu -t 1 -x P -c prints (and -c --cs for asm10) at --max-chain-skip=2147483647 for the four presets and at the
reference's default 25 for asm5 / asm10 / asm20, for MT-human x MT-orang, t-inv x q-inv and the simulated contigs (tests/asm_cases.sim_set: its seed,
parameters and md5 go to sim.json) at 0.5 %, 3 % and 8 %.  While recording it asserts: every set but asm5 at 8 % has a record and that one has
none; the asm sets contain an inversion record and one whose PAF differs between the two skips, and the reference re-chains at least one contig (map.c:698-707) under an asm preset.  The seed is
the first that gives all of it.  The reference's runs go side by side on 16 threads: one at asm20 and infinite skip takes minutes.

align_<preset>.npz: mm_align_skeleton's records and CIGAR words for the contigs at 3 %, in the layout of tests/golden/align/*.npz, the chains being
the reference's own (mg_lchain_rmq first under the asm presets) and the anchors squeezed to those the records hold (tests/asm_cases.ref_prepare).

extd2_asm_cases.npz: 200 jobs per preset over the grid of tests/ksw_cases.py at the presets' scores, answered by ksw_extd2_sse.

    python tests/tools/gen_golden_asm.py [vectors]
"""
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import align_cases as ac  # noqa: E402
import asm_cases as am  # noqa: E402
import ksw_cases as kc  # noqa: E402
import orc  # noqa: E402

LIMIT = 1024 * 1024
THREADS = 16
KSW_PER_SET, KSW_SEED = 200, 31
VARIANT_FLAGS = {"c": ["-c"], "cs": ["-c", "--cs"]}


def paf(tgt, qry, preset, skip, variant):
    exe = os.path.join(orc.REF_DIR, "minimap2_cpu")
    extra = ["--max-chain-skip=2147483647"] if skip == "inf" else []
    return subprocess.run([exe, "-t", "1", "-x", preset] + VARIANT_FLAGS[variant] + extra + [tgt, qry], check=True, capture_output=True).stdout.decode()


def write_fasta(path, recs):
    with open(path, "wb") as fh:
        for name, s in recs:
            fh.write(b">" + name.encode() + b"\n" + s + b"\n")


def record_sim(d, seed):
    """The PAFs of the simulated set at one seed, or None where the set lacks what the tests rely on."""
    meta = am.place_contigs(dict(am.SIM, seed=seed))
    if meta is None:
        return None
    refs, contigs = am.sim_set(meta)
    ref_fa = os.path.join(d, "ref.fa")
    write_fasta(ref_fa, refs)
    for tag in am.DIVS:
        write_fasta(os.path.join(d, tag + ".fa"), contigs[tag])
    cases = [c for c in am.paf_cases() if c[0].startswith("sim_")]
    with ThreadPoolExecutor(THREADS) as ex:               # (a run at asm20 and infinite skip takes minutes: all of them at once)
        texts = list(ex.map(lambda c: paf(ref_fa, os.path.join(d, c[0][4:] + ".fa"), *c[1:]), cases))
    out = {am.paf_key(*c): t for c, t in zip(cases, texts)}
    if any((t == "") != ((c[0][4:], c[1]) == am.EMPTY) for c, t in zip(cases, texts)):
        return None
    if not any("tp:A:I" in t or "tp:A:i" in t for k, t in out.items() if k.split(".")[1] in am.ASM):
        return None
    if not any(out[am.paf_key("sim_" + t, p, "inf", "c")] != out[am.paf_key("sim_" + t, p, "s25", "c")] for t in am.DIVS for p in am.ASM):
        return None                                       # the finite skip must show in some asm set's bytes
    meta["md5"] = am.sim_md5(refs, contigs)
    return meta, refs, contigs, out


def record_options_and_pafs():
    assert ac.ref_available() and os.path.exists(os.path.join(orc.REF_DIR, "minimap2_cpu")), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(am.GOLD, exist_ok=True)
    json.dump({name: am.ref_options(name) for name in am.NAMES}, open(os.path.join(am.GOLD, "options.json"), "w"), indent=1, sort_keys=True)

    cases = [c for c in am.paf_cases() if c[0] in am.PAIRS]
    with ThreadPoolExecutor(THREADS) as ex:
        texts = list(ex.map(lambda c: paf(os.path.join(ac.DATA, am.PAIRS[c[0]][0]), os.path.join(ac.DATA, am.PAIRS[c[0]][1]), *c[1:]), cases))
    pafs = {am.paf_key(*c): t for c, t in zip(cases, texts)}
    assert all((pafs[am.paf_key("mt", p, "inf", "c")] == "") == (p == "asm5") for p in am.PRESETS), "MT-human x MT-orang maps under all but asm5"
    assert all(2 <= len(pafs[am.paf_key("inv", p, "inf", "c")].splitlines()) for p in am.PRESETS)
    with tempfile.TemporaryDirectory() as d:
        for seed in range(1, 60):
            got = record_sim(d, seed)
            if got:
                break
        else:
            raise AssertionError("no seed gives the simulated set what the tests rely on")
    meta, refs, contigs, sim_pafs = got
    pafs.update(sim_pafs)
    for k, t in pafs.items():
        v = k.split(".")[3]
        assert t == "" or ("\tcg:Z:" in t and ("\tcs:Z:" in t) == (v == "cs")), k
    json.dump(meta, open(os.path.join(am.GOLD, "sim.json"), "w"), indent=1, sort_keys=True)
    path = os.path.join(am.GOLD, "pafs.npz")
    np.savez_compressed(path, **{k: np.frombuffer(t.encode(), np.uint8) for k, t in pafs.items()})
    assert os.path.getsize(path) <= LIMIT, os.path.getsize(path)
    print("seed", meta["seed"], meta["contigs"], {k: len(t.splitlines()) for k, t in pafs.items()}, os.path.getsize(path), "bytes")



def record_vectors():
    refs, contigs = am.load_sim()
    n_again = 0
    for preset in am.PRESETS:
        b, want, again = am.ref_batch([s for _, s in refs], [s for _, s in contigs["d3"]], preset)
        n_again += again if preset in am.ASM else 0
        path = os.path.join(am.GOLD, f"align_{preset}.npz")
        ac.save_batch(path, b, want)
        # the plain contig again with its anchors as the chaining left them: mm_squeeze_a inside the call then has hundreds of thousands to move
        b1, want1, _ = am.ref_batch([s for _, s in refs], [contigs["d3"][3][1]], preset, squeeze=False)
        if preset == "asm10":
            ac.save_batch(os.path.join(am.GOLD, "align_unsqueezed_asm10.npz"), b1, want1)
            assert os.path.getsize(os.path.join(am.GOLD, "align_unsqueezed_asm10.npz")) <= LIMIT
        assert sum(len(w[0]) for w in want) > 0 and os.path.getsize(path) <= LIMIT, (preset, os.path.getsize(path))
        print(preset, sum(len(w[0]) for w in want), "records,", again, "contigs re-chained,", os.path.getsize(path), "bytes")
    assert n_again > 0, "the reference re-chains no contig under an asm preset"

    rng = np.random.default_rng(KSW_SEED)
    prm, jobs, qs, ts, res, words = [], [], [], [], [], []
    for p in am.ksw_params():
        j, q, t = kc.make_batch(rng, p.m, KSW_PER_SET, kc.LENS_CPU, p_empty=0.02)
        r, w = kc.ref_batch(p, j, q, t)
        prm.append(np.array([p.m] + list(p.mat) + [p.q, p.e, p.q2, p.e2], np.int8)); jobs.append(j); qs.append(q); ts.append(t); res.append(r); words.append(w)
    ends = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    np.savez_compressed(am.KSW_GOLD, params=np.stack(prm), job_end=ends(jobs), q_end=ends(qs), t_end=ends(ts), word_end=ends(words), jobs=np.concatenate(jobs),
                        queries=np.concatenate(qs), targets=np.concatenate(ts), res=np.concatenate(res), words=np.concatenate(words))
    print(sum(len(j) for j in jobs), "DP jobs,", os.path.getsize(am.KSW_GOLD), "bytes; shares", {k: round(float(v), 3) for k, v in kc.shares(np.concatenate(res)).items()})


if __name__ == "__main__":
    if sys.argv[1:] != ["vectors"]:                       # `vectors`: the alignment and DP fixtures alone, on the recorded set (the PAFs take ten minutes)
        record_options_and_pafs()
    record_vectors()
