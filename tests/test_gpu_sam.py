"""SAM output and = / X CIGARs from the mapper (the calls named _out; minimap2 -a, --eqx, -Y, --sam-hit-only) against what the reference's CPU
program printed (tests/golden/sam/*.json.xz, recorded by tests/tools/gen_golden_sam.py): byte for byte, the header compared without @PG, for long,
short and spliced reads, with the alignment and the rewrite each on host threads and on the device -- the rewrite on the residues the alignment call
left there, and with an upload of its own.  The mapper's chaining runs on the device, so these comparisons need one whichever side the rest runs on."""
import numpy as np
import pytest

import sam_cases as sc
import mm2gb_amd as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    with mm.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import splice_cases
    import sr_cases
    out = {"long_map-ont": sc.long_inputs(str(tmp_path_factory.mktemp("sim"))), "inv": sc.inv_inputs(), "sr": ([("ref", sr_cases.gold()["genome"].encode())], sr_cases.reads()),
           "splice": splice_cases.load_pafs()[:2]}
    out["long_map-pb"] = out["long_map-ont"]
    return out


@pytest.fixture(scope="module")
def indexes(inputs):
    """One index per case for the whole module."""
    import sr_cases
    made = {}
    for case, (refs, _) in inputs.items():
        seqs = [s for _, s in refs]
        made[case] = sr_cases.index() if case == "sr" else mm.SeedIndex(seqs, **(mm.preset("splice") if case == "splice" else mm.preset("map-pb") if case.endswith("map-pb") else {}))
    yield made
    for case, ix in made.items():
        if case != "sr":
            ix.close()


RUNS = [(case, run) for case, runs in sc.CASES.items() for run in runs]


@pytest.mark.parametrize("case, run", RUNS)
def test_host_forms_equal_the_reference(engine, inputs, indexes, case, run):
    """Alignment, text and rewrite on host threads."""
    got, st = sc.map_case(engine, case, run, inputs[case], align_on_device=-1, eqx_on_device=-1, text_on_device=-1, index=indexes[case])
    sc.assert_case(got, case, run, f"{case} {run}: host forms")
    flags = [int(ln.split("\t")[1]) for ln in sc.split_sam(sc.golden(case, run))[1]] if sc.CASES[case][run][2].get("sam") else []
    reads_with_a_hit = len({ln.split("\t")[0] for ln in sc.golden(case, run).splitlines() if not ln.startswith("@") and (not flags or int(ln.split("\t")[1]) != 4)})
    assert st["n_reads"] == len(inputs[case][1]) and st["n_mapped"] == reads_with_a_hit, "n_mapped counts reads with a hit, not lines"


@pytest.mark.parametrize("case, run", [(c, r) for c, r in RUNS if sc.CASES[c][r][2].get("eqx")])
@pytest.mark.parametrize("align_on_device", [1, -1])
def test_the_device_rewrite_resident_and_uploading(engine, inputs, indexes, case, run, align_on_device):
    """eqx_on_device = 1: after the device alignment the rewrite reads the residues it left; after the host alignment it uploads them itself."""
    got, _ = sc.map_case(engine, case, run, inputs[case], align_on_device=align_on_device, eqx_on_device=1, index=indexes[case])
    sc.assert_case(got, case, run, f"{case} {run}: device rewrite, alignment {align_on_device}")


def test_defaults_and_the_device_text(engine, inputs, indexes):
    for text_on_device in (0, 1):
        got, _ = sc.map_case(engine, "long_map-ont", "a_Y_cs", inputs["long_map-ont"], text_on_device=text_on_device, index=indexes["long_map-ont"])
        sc.assert_case(got, "long_map-ont", "a_Y_cs", f"defaults, text {text_on_device}")


def test_out_none_and_zeroed_give_the_bytes_of_the_call_without_it(engine, inputs, indexes):
    refs, reads = inputs["long_map-ont"]
    names, seqs = [n for n, _ in refs], [s for _, s in refs]
    al = mm.map_align(seqs, cs="short")
    base, _ = mm.map_reads(engine, indexes["long_map-ont"], names, reads, align=al)
    assert base and "\tcg:Z:" in base and "M" in base.split("\tcg:Z:")[1].split("\t")[0]
    for out in (None, mm.map_out()):
        got, _ = mm.map_reads(engine, indexes["long_map-ont"], names, reads, align=al, out=out)
        assert got == base
    got, _ = mm.map_reads(engine, indexes["long_map-ont"], names, reads, align=al, out=mm.map_out(softclip=True, hit_only=True))
    assert got == base, "-Y and --sam-hit-only mean nothing in PAF"


@pytest.mark.parametrize("case, run, chunk", [("long_map-ont", "a_eqx", 12_000), ("sr", "a", 5_000), ("splice", "a_eqx", 12_000)])
def test_a_stream_of_chunks(engine, inputs, indexes, case, run, chunk):
    with mm.Engine() as e2:
        got, st = sc.map_case([engine, e2], case, run, inputs[case], stream=chunk, index=indexes[case])
    sc.assert_case(got, case, run, f"{case} {run}: stream")
    assert st["n_reads"] == len(inputs[case][1])


def test_a_refused_call_leaves_the_engine_usable(engine, inputs, indexes):
    refs, reads = inputs["inv"]
    names, seqs = [n for n, _ in refs], [s for _, s in refs]
    out = mm.map_out(sam=True)
    out.format = 2
    with pytest.raises(mm.Mm2gbError, match="format is 0 .PAF. or 1 .SAM."):
        mm.map_reads(engine, indexes["inv"], names, reads, align=mm.map_align(seqs), out=out)
    out = mm.map_out(sam=True)
    out.flag |= mm.F_SPLICE
    with pytest.raises(mm.Mm2gbError, match="MM_F_EQX, MM_F_SOFTCLIP and MM_F_SAM_HIT_ONLY"):
        mm.map_reads(engine, indexes["inv"], names, reads, align=mm.map_align(seqs), out=out)
    with pytest.raises(mm.Mm2gbError, match="MM_F_EQX"):          # the alignment options keep refusing the bit: it belongs to map_out
        mm.map_reads(engine, indexes["inv"], names, reads, align=mm.map_align(seqs, flag=mm.F_EQX), out=mm.map_out(sam=True))
    with pytest.raises(mm.Mm2gbError, match="only MM_F_FOR_ONLY and MM_F_REV_ONLY"):
        mm.map_reads(engine, indexes["inv"], names, reads, opt=mm.map_opt(flag=mm.F_EQX), align=mm.map_align(seqs), out=mm.map_out(sam=True))
    got, _ = sc.map_case(engine, "inv", "a", inputs["inv"], eqx_on_device=1, index=indexes["inv"])
    sc.assert_case(got, "inv", "a", "a good call after the refusals")
