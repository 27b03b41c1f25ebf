"""The resident path's fixture without a GPU (tests/golden/resident, tests/resident_cases.py): that it holds what tests/test_gpu_resident.py relies on -- the
conditions tests/tools/gen_golden_resident.py asserted while recording -- that the chimeric set is the one the seed gives, and, where the reference program is
built (oracle/_ref), that it prints the recorded text today."""
import os
import subprocess

import pytest

import orc
import resident_cases as rc

EXE = os.path.join(orc.REF_DIR, "minimap2_cpu")
needs_ref = pytest.mark.skipif(not os.path.exists(EXE), reason="the reference build (oracle/_ref) is not here")
KEYS = [f"{run}.{skip}" for run in rc.RUNS for skip in rc.SKIPS]


def test_the_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(rc.GOLD, "resident.npz")) < 1024 * 1024
    g = rc.gold()
    assert sorted(g["paf"]) == sorted(KEYS) and set(g) == {"seed", "ref", "reads", "paf", "moved", "tp_S"}
    assert sorted(g["moved"]) == sorted(k for k in KEYS if k.startswith("chim.")) and sorted(g["tp_S"]) == sorted(k for k in KEYS if k.startswith("sim160."))


def test_the_chimeric_set_is_the_seeds():
    genome, reads = rc.sim_chim(rc.gold()["seed"])
    assert rc.gold()["seed"] == rc.CHIM_SEED and rc.refs_of("chim") == [("chim_ref", genome)] and rc.reads_of("chim") == reads
    assert len(genome) == 120_000 and len(reads) == 61 and reads[-1][0] == "stray"
    assert genome[100_000:100_090] * 40 == genome[100_000:103_600] and genome[20_000:28_000] != genome[70_000:78_000]


@pytest.mark.parametrize("key", [k for k in KEYS if k.startswith("chim.")])
def test_chimeric_runs_drop_records_and_keep_some_at_a_moved_place(key):
    """What the generator counted against the same run with -P, and what shows without that run: reads with several lines, both strands, a read with none."""
    g = rc.gold()
    rows = [ln.split("\t") for ln in g["paf"][key].splitlines()]
    assert g["moved"][key] >= rc.MIN_MOVED
    names = [n for n, _ in rc.reads_of("chim")]
    assert set(names) - {f[0] for f in rows} and {f[0] for f in rows} <= set(names)                   # a read without a line
    assert sum("tp:A:P" in f for f in rows) >= 60 and sum(sum(f[0] == n for f in rows) > 1 for n in names) >= 20              # the chimeric reads' pieces: several lines each
    assert all(any(t.startswith("dv:f:") for t in f[12:]) for f in rows)
    assert sum(f[4] == "-" for f in rows) >= 10 and sum(f[4] == "+" for f in rows) >= 10


@pytest.mark.parametrize("key", [k for k in KEYS if k.startswith("sim160.")])
def test_sim160_runs_hold_secondary_lines_and_a_read_without_a_line(key):
    g = rc.gold()
    rows = [ln.split("\t") for ln in g["paf"][key].splitlines()]
    assert g["tp_S"][key] == sum("tp:A:S" in f for f in rows) >= rc.MIN_TP_S
    names = [n for n, _ in rc.reads_of("sim160")]
    assert len(names) == 161 and set(names) - {f[0] for f in rows} == {"stray"}


def test_moved_reads_on_a_small_example():
    """The generator's count on text written by hand: read a keeps the chain that was third at the second place and the second chain had another dv (counted);
    read b keeps its chains where they were; read c's moved record meets the same dv at its new place (not counted)."""
    ln = lambda q, s, dv: "\t".join([q, "100", str(s), "90", "+", "t", "1000", str(s), "90", "50", "60", "0", "tp:A:P", f"dv:f:{dv}"]) + "\n"
    all_chains = ln("a", 1, "0.01") + ln("a", 2, "0.02") + ln("a", 3, "0.03") + ln("b", 1, "0.01") + ln("b", 2, "0.02") + ln("c", 1, "0.01") + ln("c", 2, "0.05") + ln("c", 3, "0.05")
    kept = ln("a", 1, "0.01") + ln("a", 3, "0.03") + ln("b", 1, "0.01") + ln("b", 2, "0.02") + ln("c", 1, "0.01") + ln("c", 3, "0.05")
    assert rc.moved_reads(kept, all_chains) == ["a"]
    assert rc.moved_reads(all_chains, all_chains) == []


def test_the_skip_limit_and_the_bandwidth_show_in_the_bytes():
    assert any(rc.golden_paf(run, "s25") != rc.golden_paf(run, "inf") for run in rc.RUNS)
    assert rc.golden_paf("chim.map-ont", "inf") != rc.golden_paf("chim.map-pb", "inf")


@needs_ref
@pytest.mark.parametrize("key", KEYS)
def test_the_reference_program_prints_the_recorded_text(key, tmp_path_factory):
    name, kind, skip = key.split(".")
    d = tmp_path_factory.getbasetemp() / f"resident_{name}"
    tgt, qry = str(d / "ref.fa"), str(d / "reads.fa")
    if not d.exists():
        d.mkdir()
        for path, recs in ((tgt, rc.refs_of(name)), (qry, rc.reads_of(name))):
            with open(path, "wb") as fh:
                for n, s in recs:
                    fh.write(b">" + n.encode() + b"\n" + s + b"\n")
    got = subprocess.run([EXE, "-t", "1"] + rc.KINDS[kind][0] + [f"--max-chain-skip={rc.SKIPS[skip]}", tgt, qry], check=True, capture_output=True).stdout.decode()
    assert got == rc.gold()["paf"][key]
