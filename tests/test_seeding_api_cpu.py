"""The public face of seeding on the device (mm2gb_sketch_gpu, mm2gb_collect_matches_gpu, map_opt(seeding_on_device=...)) as far as it can be
checked without a GPU: the option's place and default, and the argument checks that come before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

mm = pytest.importorskip("mm2gb_amd")


def test_option_is_last_and_off_and_entry_points_refuse_a_null_engine():
    o = mm.map_opt()
    assert mm.MapOpt._fields_[-1][0] == "seeding_on_device" and o.seeding_on_device == 0
    assert o.max_chain_skip == 2**31 - 1 and o.seeds_on_device == 0
    assert mm.map_opt(seeding_on_device=1).seeding_on_device == 1
    L = mm.lib()
    off = np.zeros(2, np.int64); off[1] = 4
    mini_off = np.zeros(2, np.int64)
    ptr = C.c_void_p()
    assert L.mm2gb_sketch_gpu(None, 10, 15, 1, off.ctypes.data, b"ACGT", None, mini_off.ctypes.data, C.byref(ptr)) != 0
    assert "mm2gb_sketch_gpu" in L.mm2gb_last_error().decode()
    opt = mm.SeedOpt(10, 4095, 500, 0.01)
    m = mm.MatchBatch()
    with mm.SeedIndex([b"ACGTTGCATGCCATGA" * 20]) as ix:
        assert L.mm2gb_collect_matches_gpu(None, ix._h, C.byref(opt), 1, off.ctypes.data, b"ACGT", C.byref(m)) != 0
        assert "mm2gb_collect_matches_gpu" in L.mm2gb_last_error().decode()
    assert L.mm2gb_index_to_device(None, 0) != 0
    assert "mm2gb_index_to_device" in L.mm2gb_last_error().decode()
    L.mm2gb_match_batch_free(C.byref(m))                    # an empty record is fine to free
