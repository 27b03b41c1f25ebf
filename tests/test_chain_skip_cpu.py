"""The chaining DP's opt-in skip limit, what can be checked without a GPU: the C ABI exports the mode, the mapper's options carry
max_chain_skip (default: infinity, the GPU path's contract), and the CPU oracle that the GPU tests compare against really does
give the reference's recorded results at the finite limits the golden vectors were made with."""
import numpy as np
import pytest

import golden_io
import orc

mm = pytest.importorskip("mm2gb_amd")

FINITE = [p for p in golden_io.all_cases() if golden_io.load(p)["prm"].max_skip != orc.INT32_MAX]


def test_the_abi_has_the_mode():
    L = mm.lib()
    for name in ("mm2gb_engine_set_chain_skip", "mm2gb_engine_last_score_form"):
        assert hasattr(L, name)
    assert L.mm2gb_engine_set_chain_skip(None, 1) < 0          # no engine: an error, not a crash
    assert L.mm2gb_engine_last_score_form(None) == -1
    assert hasattr(mm.Engine, "set_chain_skip") and hasattr(mm.Engine, "last_score_form")


def test_map_opt_carries_max_chain_skip():
    o = mm.map_opt()
    assert o.max_chain_skip == orc.INT32_MAX                   # mm2gb_map_opt_init wrote it: the Python mirror has the C layout
    assert mm.map_opt(max_chain_skip=25).max_chain_skip == 25


# The two tests below check the fixtures the GPU tests rest on (the oracle and the golden vectors at finite limits), not the new mode:
# they pass without it too.


def test_there_are_finite_limit_vectors():
    names = golden_io.case_ids(FINITE)
    assert "synth_skip0" in names and "synth_skip25" in names and any(n.startswith("real_mt_s25") for n in names)


@pytest.mark.parametrize("path", FINITE, ids=golden_io.case_ids(FINITE))
def test_oracle_keeps_the_limit(path):
    g = golden_io.load(path)
    f, p, _ = orc.chain_fill(g["a"], g["prm"])
    assert np.array_equal(f, g["f"]) and np.array_equal(p, g["p"])
    prm = g["prm"]
    prm.max_skip = orc.INT32_MAX
    fi, pi, _ = orc.chain_fill(g["a"], prm)
    if g["name"] == "synth_skip0":          # at least one vector that tells the two modes apart
        assert not (np.array_equal(fi, g["f"]) and np.array_equal(pi, g["p"]))
