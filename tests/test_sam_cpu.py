"""SAM output and = / X CIGARs from the mapper, what can be checked without a GPU: what the recorded runs of the reference program hold
(tests/golden/sam/*.json.xz), the header call, map_out's values, and the refusals, which are made before the call looks for its engine.  The mapper
itself chains on the device: its bytes are compared in tests/test_gpu_sam.py, on host threads and on the device."""
import re
import types

import pytest

import mm2gb_amd as mm
import sam_cases as sc


def rows(case, run):
    return [ln.split("\t") for ln in sc.golden(case, run).splitlines() if not ln.startswith("@")]


def test_the_long_read_runs_hold_what_the_tests_rely_on():
    for case in ("long_map-ont", "long_map-pb"):
        a, eqx, y, hit = rows(case, "a"), rows(case, "a_eqx"), rows(case, "a_Y_cs"), rows(case, "a_md_hit")
        assert any(int(r[1]) & 0x100 and r[9] == "*" for r in a), "a 0x100 line with SEQ *"
        assert any(int(r[1]) & 0x10 for r in a) and any("\tzd:i:" in "\t".join(r) for r in a)
        assert [r[0] for r in a if int(r[1]) == 4] == [sc.UNMAPPED] and not any(int(r[1]) == 4 for r in hit), "a flag-4 line that --sam-hit-only leaves out"
        assert len(hit) == len(a) - 1 and all(any(f.startswith("MD:Z:") for f in r) for r in hit)
        assert any("=" in r[5] and "X" in r[5] for r in eqx) and not any("M" in r[5] for r in eqx)
        assert all(any(f.startswith("cs:Z:") for f in r) for r in y if int(r[1]) != 4)
        assert all(r[-1].startswith("rl:i:") for r in a + y), "rl:i comes last, after cs:Z"
        for run in ("c_eqx", "c_eqx_cs"):
            p = rows(case, run)
            assert all(any(f.startswith("cg:Z:") and "=" in f and "M" not in f[5:] for f in r) for r in p)
            assert all(any(f.startswith("cs:Z:") for f in r) for r in p) == (run == "c_eqx_cs")
        assert sc.golden(case, "a").startswith("@SQ\tSN:chr1\tLN:100000\n")


def test_supplementary_lines_clips_and_introns_are_in_the_other_runs():
    """The simulated long reads have no chimera: 0x800 lines with SA:Z and the H / S clips come from t-inv x q-inv, the short and the spliced reads."""
    a, y = rows("inv", "a"), rows("inv", "a_Y")
    assert "tp:A:I" in sc.golden("inv", "a") or "tp:A:i" in sc.golden("inv", "a")
    assert any(int(r[1]) & 0x800 and "H" in r[5] and "S" in s[5] and "H" not in s[5] and len(s[9]) > len(r[9]) for r, s in zip(a, y)), "H clips without -Y, S clips with it"
    for case, run in (("inv", "a"), ("sr", "a"), ("splice", "a_cs")):
        r_ = rows(case, run)
        supp = {r[0] for r in r_ if int(r[1]) & 0x800}
        assert supp and all(any(f.startswith("SA:Z:") for f in r) for r in r_ if r[0] in supp and int(r[1]) & 0x900 == 0), f"{case}: a 0x800 line and SA:Z on its read's primary line"
    assert any(int(r[1]) == 4 for r in rows("sr", "a")) and not any(int(r[1]) & 0x100 for r in rows("sr", "a"))
    assert any(re.search(r"=\d+N\d+=", r[5]) for r in rows("splice", "a_eqx")), "an N word between = words"
    assert "~" in sc.golden("splice", "a_cs") and "\tts:A:" in sc.golden("splice", "a_cs")


def test_sam_header():
    assert mm.sam_header(["chr1", "b"], [100, 7]) == "@SQ\tSN:chr1\tLN:100\n@SQ\tSN:b\tLN:7\n@PG\tID:mm2-gb_amd\tPN:mm2-gb_amd\n"
    assert mm.sam_header([], []) == "@PG\tID:mm2-gb_amd\tPN:mm2-gb_amd\n"
    with pytest.raises(mm.Mm2gbError, match="one length per name"):
        mm.sam_header(["a"], [])
    want = sc.split_sam(sc.golden("splice", "a_cs"))[0]
    import splice_cases
    refs = splice_cases.load_pafs()[0]
    assert sc.split_sam(mm.sam_header([n for n, _ in refs], [len(s) for _, s in refs]))[0] == want


def test_map_out_values():
    o = mm.map_out()
    assert (o.format, o.flag, o.eqx_on_device) == (0, 0, 0)
    o = mm.map_out(sam=True, eqx=True, softclip=True, hit_only=True, eqx_on_device=-1)
    assert (o.format, o.flag, o.eqx_on_device) == (1, 0x4000000 | 0x80000 | 0x40000000, -1)
    assert (mm.F_EQX, mm.F_SOFTCLIP, mm.F_SAM_HIT_ONLY) == (0x4000000, 0x80000, 0x40000000)


def test_refusals_by_name():
    """The options are looked at before anything else: nothing runs, not even the look for an engine (the handle here is null)."""
    no_engine = types.SimpleNamespace(_h=None)
    refs = [b"ACGT" * 300]
    reads = [("q", b"ACGT" * 100)]
    with mm.SeedIndex(refs, k=15, w=10, threads=1) as ix:
        for out in (mm.map_out(sam=True), mm.map_out(eqx=True)):
            with pytest.raises(mm.Mm2gbError, match="need base-level alignment"):
                mm.map_reads(no_engine, ix, ["t"], reads, out=out)
            with pytest.raises(mm.Mm2gbError, match="need base-level alignment"):
                mm.map_reads_stream([no_engine], ix, ["t"], reads, out=out)
            with pytest.raises(mm.Mm2gbError, match="mm2gb_map_reads_sr_out: .* needs base-level alignment"):
                mm.map_reads(no_engine, ix, ["t"], reads, opt=mm.map_opt_sr(), k=21, align=mm.map_sr(), out=out)
        for bit, name in ((mm.F_ALL_CHAINS, "MM_F_ALL_CHAINS"), (mm.F_NO_DIAG, "MM_F_NO_DIAG"), (mm.F_NO_DUAL, "MM_F_NO_DUAL")):
            with pytest.raises(mm.Mm2gbError, match=f"{name} is not supported with base-level alignment"):
                mm.map_reads(no_engine, ix, ["t"], reads, opt=mm.map_opt(flag=bit | mm.F_NO_LJOIN), align=mm.map_align(refs), out=mm.map_out(sam=True))
        bad = mm.map_out(sam=True)
        bad.format = 3
        with pytest.raises(mm.Mm2gbError, match="mm2gb_map_reads_aln_out: format is 0"):
            mm.map_reads(no_engine, ix, ["t"], reads, align=mm.map_align(refs), out=bad)
        bad = mm.map_out(sam=True)
        bad.flag |= 0x8
        with pytest.raises(mm.Mm2gbError, match="mm2gb_map_reads_splice_out: .*only MM_F_EQX, MM_F_SOFTCLIP and MM_F_SAM_HIT_ONLY"):
            mm.map_reads(no_engine, ix, ["t"], reads, opt=mm.map_opt_splice(), align=mm.map_splice(refs), out=bad)
        # the existing calls keep refusing MM_F_EQX in the mapping options, with or without out
        for out in (None, mm.map_out(sam=True)):
            with pytest.raises(mm.Mm2gbError, match="only MM_F_FOR_ONLY and MM_F_REV_ONLY are supported"):
                mm.map_reads(no_engine, ix, ["t"], reads, opt=mm.map_opt(flag=mm.F_EQX), align=mm.map_align(refs), out=out)
        # a good set of output options gets as far as looking for its engine
        with pytest.raises(mm.Mm2gbError, match="null argument"):
            mm.map_reads(no_engine, ix, ["t"], reads, align=mm.map_align(refs), out=mm.map_out(sam=True, eqx=True))
