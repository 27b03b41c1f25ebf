"""mm2-gb chaining on MI355X: thin ctypes plumbing over libmm2gb_chain.so (HIP kernels + C ABI, include/mm2gb_chain.h).

The directory name carries a hyphen, so load it with
    importlib.import_module("mm2-gb_amd")
(or use the `mm2gb_amd` shim module at the repository root).

There is no CPU fallback: if the shared library is missing or no GPU is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MM2GB_LIB_PATH") or os.path.join(_HERE, "libmm2gb_chain.so")   # override: A/B runs of kernel builds
INT32_MAX = 2**31 - 1


class Misc(C.Structure):
    """mm2gb_misc_t == Misc (gpu/plutils.h:33-37)."""
    _fields_ = [("max_iter", C.c_int), ("max_dist_x", C.c_int), ("max_dist_y", C.c_int), ("max_skip", C.c_int),
                ("bw", C.c_int), ("min_cnt", C.c_int), ("min_score", C.c_int), ("is_cdna", C.c_int), ("n_seg", C.c_int),
                ("chn_pen_gap", C.c_float), ("chn_pen_skip", C.c_float)]


class _RangeCfg(C.Structure):
    _fields_ = [("blockdim", C.c_int), ("cut_check_anchors", C.c_int), ("anchor_per_block", C.c_int)]


class _ScoreCfg(C.Structure):
    _fields_ = [("micro_batch", C.c_int), ("mid_blockdim", C.c_int), ("short_griddim", C.c_int), ("long_griddim", C.c_int),
                ("mid_griddim", C.c_int), ("long_seg_cutoff", C.c_int), ("mid_seg_cutoff", C.c_int)]


class Config(C.Structure):
    """mm2gb_config_t: the gpu_config.json schema (gpu/gpu_config.json)."""
    _fields_ = [("num_streams", C.c_int), ("min_n", C.c_int), ("long_seg_buffer_size", C.c_int64), ("max_total_n", C.c_int64),
                ("max_read", C.c_int), ("avg_read_n", C.c_int),
                ("has_max_total_n", C.c_int), ("has_max_read", C.c_int), ("has_avg_read_n", C.c_int),
                ("range_kernel", _RangeCfg), ("score_kernel", _ScoreCfg)]


class Stats(C.Structure):
    _fields_ = [("n_anchors", C.c_int64), ("n_reads", C.c_int64), ("n_pairs", C.c_int64), ("n_chunks", C.c_int64),
                ("n_long_chunks", C.c_int64), ("n_mid_chunks", C.c_int64), ("n_tracked_chunks", C.c_int64), ("n_clamped_blocks", C.c_int64),
                ("ms_h2d", C.c_float), ("ms_prep", C.c_float), ("ms_score", C.c_float), ("ms_d2h", C.c_float), ("ms_total", C.c_float),
                ("ms_post", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Chains(C.Structure):
    _fields_ = [("u_off", C.POINTER(C.c_int64)), ("u", C.POINTER(C.c_uint64)), ("a_off", C.POINTER(C.c_int64)), ("a", C.c_void_p)]


class RmqParam(C.Structure):
    """mm2gb_rmq_param_t == the leading arguments of mg_lchain_rmq (lchain.c:250-251)."""
    _fields_ = [("max_dist", C.c_int), ("max_dist_inner", C.c_int), ("bw", C.c_int), ("max_chn_skip", C.c_int), ("cap_rmq_size", C.c_int),
                ("min_cnt", C.c_int), ("min_sc", C.c_int), ("chn_pen_gap", C.c_float), ("chn_pen_skip", C.c_float)]


READ_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_uint64), C.c_int64, C.c_void_p)


class BatcherStats(C.Structure):
    _fields_ = [("reads", C.c_int64), ("anchors", C.c_int64), ("reads_per_lane", C.c_int64 * 2), ("batches", C.c_int64 * 2),
                ("batches_per_engine", C.c_int64 * 16), ("n_engines", C.c_int)]


class Mm2gbError(RuntimeError):
    pass


_lib = None

# every symbol include/mm2gb_chain.h and include/mm2gb_plutils.h declare
CORE_SYMBOLS = ["mm2gb_last_error", "mm2gb_version", "mm2gb_config_defaults", "mm2gb_config_parse", "mm2gb_config_load",
                "mm2gb_device_count", "mm2gb_device_numa_node", "mm2gb_pin_thread_to_device", "mm2gb_numa_cpus_for_bdf", "mm2gb_engine_create", "mm2gb_engine_destroy", "mm2gb_engine_set_misc", "mm2gb_engine_device", "mm2gb_engine_cu_count", "mm2gb_engine_gang_counts", "mm2gb_has_gang_build",
                "mm2gb_engine_reserve", "mm2gb_score_host", "mm2gb_score_device", "mm2gb_engine_sync", "mm2gb_engine_stats",
                "mm2gb_engine_stream", "mm2gb_engine_last_kernel_ms", "mm2gb_chain_host", "mm2gb_chain_gpu", "mm2gb_post_device", "mm2gb_post_device_enqueue", "mm2gb_post_device_totals", "mm2gb_post_device_digest", "mm2gb_chains_free", "mm2gb_backtrack_host",
                "mm2gb_free", "mm2gb_lchain_dp", "mm2gb_synth_count", "mm2gb_synth_fill",
                "mm2gb_pool_create", "mm2gb_pool_destroy", "mm2gb_pool_size", "mm2gb_pool_device", "mm2gb_pool_set_misc",
                "mm2gb_pool_score_host", "mm2gb_pool_chain_host",
                "mm2gb_batcher_create", "mm2gb_batcher_add", "mm2gb_batcher_feed", "mm2gb_batcher_flush", "mm2gb_batcher_stats", "mm2gb_batcher_destroy",
                "mm2gb_plan_batches", "mm2gb_rmq_chain_gpu", "mm2gb_lchain_rmq", "mm2gb_lchain_rmq_counts",
                "mm2gb_sort_seeds_gpu", "mm2gb_gen_regs_gpu", "mm2gb_collect_seeds_gpu",
                "mm2gb_sketch", "mm2gb_index_build", "mm2gb_index_destroy", "mm2gb_index_size", "mm2gb_index_mid_occ", "mm2gb_collect_matches", "mm2gb_matches_free", "mm2gb_map_opt_init", "mm2gb_map_reads", "mm2gb_engine_release_host_scratch", "mm2gb_rmq_chain_host", "mm2gb_rmq_chain_host_tied", "mm2gb_rmq_chain", "mm2gb_engine_set_rmq_kernel", "mm2gb_engine_set_rmq_team_reads", "mm2gb_engine_set_chain_skip", "mm2gb_engine_last_score_form", "mm2gb_engine_last_score_mode", "mm2gb_engine_band_groups", "mm2gb_engine_band_shape", "mm2gb_collect_seeds_host", "mm2gb_map_reads_multi", "mm2gb_map_reads_stream",
                "mm2gb_sketch_gpu", "mm2gb_index_to_device", "mm2gb_collect_matches_gpu", "mm2gb_match_batch_free",
                "mm2gb_index_build_gpu", "mm2gb_index_mid_occ_gpu", "mm2gb_index_view", "mm2gb_index_fetch_device", "mm2gb_index_build_split",
                "mm2gb_sketch_flag", "mm2gb_sketch_gpu_flag", "mm2gb_index_build_flag", "mm2gb_index_build_gpu_flag", "mm2gb_index_flag",
                "mm2gb_align_opt_init", "mm2gb_align_regs_host", "mm2gb_align_regs_gpu", "mm2gb_align_out_free",
                "mm2gb_align_splice_opt_init", "mm2gb_align_regs_splice_host", "mm2gb_align_regs_splice_gpu", "mm2gb_aln_text_splice_host", "mm2gb_aln_text_splice_gpu",
                "mm2gb_map_opt_init_splice", "mm2gb_map_reads_splice", "mm2gb_map_reads_stream_splice", "mm2gb_map_opt_init_preset",
                "mm2gb_ksw_extz2_host", "mm2gb_ksw_extz2_gpu", "mm2gb_align_regs_extz_host", "mm2gb_align_regs_extz_gpu",
                "mm2gb_map_opt_init_sr", "mm2gb_collect_seeds_heap_host", "mm2gb_collect_seeds_heap_gpu", "mm2gb_map_sr_init", "mm2gb_map_reads_sr",
                "mm2gb_cigar_eqx_host", "mm2gb_cigar_eqx_gpu", "mm2gb_cigar_eqx_gpu_info", "mm2gb_map_out_init", "mm2gb_sam_header",
                "mm2gb_map_reads_aln_out", "mm2gb_map_reads_stream_aln_out", "mm2gb_map_reads_splice_out", "mm2gb_map_reads_stream_splice_out",
                "mm2gb_map_reads_sr_out", "mm2gb_map_reads_stream_sr_out",
                "mm2gb_collect_matches_frag", "mm2gb_collect_matches_frag_gpu", "mm2gb_frag_offsets", "mm2gb_map_frags_sr", "mm2gb_map_frags_stream_sr",
                "mm2gb_select_sub_multi_host", "mm2gb_seg_gen_host", "mm2gb_seg_out_free"]
BOUNDARY_SYMBOLS = ["init_stream_gpu", "chain_stream_gpu", "finish_stream_gpu", "free_stream_gpu"]


def lib():
    """Load libmm2gb_chain.so (built in-tree by `make -C mm2-gb_amd` / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Mm2gbError(f"{LIB_PATH} is missing: build it with `make -C {_HERE}` (hipcc, --offload-arch=gfx950); "
                             "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.mm2gb_last_error.restype = C.c_char_p
        L.mm2gb_version.restype = C.c_char_p
        L.mm2gb_config_defaults.argtypes = [C.POINTER(Config)]
        L.mm2gb_config_defaults.restype = None
        L.mm2gb_config_parse.argtypes = [C.c_char_p, C.POINTER(Config)]
        L.mm2gb_config_load.argtypes = [C.c_char_p, C.POINTER(Config)]
        L.mm2gb_engine_create.restype = C.c_void_p
        L.mm2gb_engine_create.argtypes = [C.POINTER(Config), C.POINTER(Misc), C.c_int]
        L.mm2gb_engine_destroy.argtypes = [C.c_void_p]
        L.mm2gb_engine_destroy.restype = None
        L.mm2gb_engine_set_misc.argtypes = [C.c_void_p, C.POINTER(Misc)]
        L.mm2gb_engine_device.argtypes = [C.c_void_p]
        L.mm2gb_engine_reserve.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
        L.mm2gb_engine_set_chain_skip.argtypes = [C.c_void_p, C.c_int]
        L.mm2gb_engine_last_score_form.argtypes = [C.c_void_p]
        L.mm2gb_engine_last_score_mode.argtypes = [C.c_void_p]
        L.mm2gb_engine_band_groups.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.mm2gb_score_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.mm2gb_score_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.mm2gb_engine_sync.argtypes = [C.c_void_p]
        L.mm2gb_engine_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.mm2gb_engine_stream.argtypes = [C.c_void_p]
        L.mm2gb_engine_stream.restype = C.c_void_p
        L.mm2gb_engine_last_kernel_ms.argtypes = [C.c_void_p]
        L.mm2gb_engine_last_kernel_ms.restype = C.c_float
        L.mm2gb_chain_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Chains), C.POINTER(Stats)]
        L.mm2gb_chain_gpu.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(Chains), C.POINTER(Stats)]
        L.mm2gb_post_device_enqueue.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.mm2gb_post_device_totals.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.mm2gb_post_device_digest.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.mm2gb_post_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.mm2gb_chains_free.argtypes = [C.POINTER(Chains)]
        L.mm2gb_chains_free.restype = None
        L.mm2gb_backtrack_host.argtypes = [C.POINTER(Misc), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.mm2gb_free.argtypes = [C.c_void_p]
        L.mm2gb_free.restype = None
        L.mm2gb_lchain_dp.restype = C.c_void_p
        L.mm2gb_lchain_dp.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                                      C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p]
        L.mm2gb_synth_count.restype = C.c_int64
        L.mm2gb_synth_count.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        L.mm2gb_synth_fill.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.mm2gb_pool_create.restype = C.c_void_p
        L.mm2gb_pool_create.argtypes = [C.POINTER(Config), C.POINTER(Misc), C.c_int, C.c_void_p]
        L.mm2gb_pool_destroy.argtypes = [C.c_void_p]
        L.mm2gb_pool_destroy.restype = None
        L.mm2gb_pool_size.argtypes = [C.c_void_p]
        L.mm2gb_pool_device.argtypes = [C.c_void_p, C.c_int]
        L.mm2gb_pool_set_misc.argtypes = [C.c_void_p, C.POINTER(Misc)]
        L.mm2gb_pool_score_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats), C.c_void_p]
        L.mm2gb_pool_chain_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Chains), C.POINTER(Stats)]
        L.mm2gb_rmq_chain_gpu.argtypes = [C.c_void_p, C.POINTER(RmqParam), C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(Chains), C.c_void_p, C.POINTER(Stats)]
        L.mm2gb_lchain_rmq.restype = C.c_void_p
        L.mm2gb_lchain_rmq.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p]
        L.mm2gb_lchain_rmq_counts.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mm2gb_lchain_rmq_counts.restype = None
        L.mm2gb_sort_seeds_gpu.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.mm2gb_sketch.argtypes = [C.c_char_p, C.c_int32, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.mm2gb_sketch_flag.argtypes = [C.c_char_p, C.c_int32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.mm2gb_index_build_flag.restype = C.c_void_p
        L.mm2gb_index_build_flag.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_int]
        L.mm2gb_index_build_gpu_flag.restype = C.c_void_p
        L.mm2gb_index_build_gpu_flag.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p]
        L.mm2gb_index_flag.argtypes = [C.c_void_p]
        L.mm2gb_sketch_gpu_flag.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mm2gb_index_build.restype = C.c_void_p
        L.mm2gb_index_build.argtypes = [C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_int]
        L.mm2gb_index_destroy.restype = None
        L.mm2gb_index_destroy.argtypes = [C.c_void_p]
        L.mm2gb_index_size.restype = C.c_int64
        L.mm2gb_index_size.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.mm2gb_index_mid_occ.restype = C.c_int32
        L.mm2gb_index_mid_occ.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_int32]
        L.mm2gb_index_build_gpu.restype = C.c_void_p
        L.mm2gb_index_build_gpu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p]
        L.mm2gb_index_mid_occ_gpu.restype = C.c_int32
        L.mm2gb_index_mid_occ_gpu.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_int32]
        L.mm2gb_index_view.argtypes = [C.c_void_p, C.c_void_p]
        L.mm2gb_index_fetch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mm2gb_index_build_split.argtypes = [C.c_void_p, C.c_void_p]
        L.mm2gb_collect_matches.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.mm2gb_matches_free.restype = None
        L.mm2gb_matches_free.argtypes = [C.c_void_p]
        L.mm2gb_sketch_gpu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mm2gb_index_to_device.argtypes = [C.c_void_p, C.c_int]
        L.mm2gb_collect_matches_gpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_char_p, C.c_void_p]
        L.mm2gb_match_batch_free.restype = None
        L.mm2gb_match_batch_free.argtypes = [C.c_void_p]
        L.mm2gb_collect_seeds_gpu.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mm2gb_gen_regs_gpu.argtypes = [C.c_void_p, C.c_int64, C.POINTER(Chains), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mm2gb_batcher_create.restype = C.c_void_p
        L.mm2gb_batcher_create.argtypes = [C.POINTER(Config), C.POINTER(Misc), C.c_int, C.c_void_p, C.c_int, READ_DONE_FN, C.c_void_p]
        L.mm2gb_batcher_add.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.mm2gb_batcher_flush.argtypes = [C.c_void_p]
        L.mm2gb_batcher_stats.argtypes = [C.c_void_p, C.POINTER(BatcherStats)]
        L.mm2gb_batcher_destroy.argtypes = [C.c_void_p]
        L.mm2gb_batcher_destroy.restype = None
        L.mm2gb_plan_batches.restype = C.c_int64
        L.mm2gb_plan_batches.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise Mm2gbError(lib().mm2gb_last_error().decode())


def default_misc(**kw):
    """build_misc() for map-ont / no preset (map.c:393-426; options.c:24-36; k = 15)."""
    d = dict(max_iter=5000, max_dist_x=5000, max_dist_y=5000, max_skip=INT32_MAX, bw=500, min_cnt=3, min_score=40,
             is_cdna=0, n_seg=1, chn_pen_gap=np.float32(0.8 * 0.01 * 15), chn_pen_skip=np.float32(0.0))
    d.update(kw)
    return Misc(**d)


def default_config():
    c = Config()
    lib().mm2gb_config_defaults(C.byref(c))
    return c


def parse_config(text):
    c = Config()
    _check(lib().mm2gb_config_parse(text.encode(), C.byref(c)))
    return c


def load_config(path):
    c = Config()
    _check(lib().mm2gb_config_load(os.fsencode(path), C.byref(c)))
    return c


def device_count():
    return lib().mm2gb_device_count()


def device_numa_node(device):
    """NUMA node of the device's PCIe root (-1: unknown)."""
    return lib().mm2gb_device_numa_node(int(device))


def pin_thread_to_device(device):
    """Move the calling thread (and the threads it starts afterwards) onto the usable CPUs of the device's NUMA node; 0 = nothing changed."""
    return lib().mm2gb_pin_thread_to_device(int(device))


def numa_cpus_for_bdf(bdf, sysfs_root=""):
    """(node, cpus) of a PCI device from a sysfs tree (tests hand in a made-up one)."""
    L = lib()
    L.mm2gb_numa_cpus_for_bdf.restype = C.c_int
    L.mm2gb_numa_cpus_for_bdf.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]
    node = C.c_int32(-1)
    buf = (C.c_int32 * 4096)()
    n = L.mm2gb_numa_cpus_for_bdf(bdf.encode(), sysfs_root.encode(), C.byref(node), buf, 4096)
    return node.value, list(buf[:min(n, 4096)])


class Engine:
    """One chaining engine on one GPU (mm2gb_engine_t)."""

    def __init__(self, misc=None, config=None, device=0, chain_skip=None):
        """chain_skip: True keeps misc.max_skip in the chaining DP (mg_lchain_dp's results at that limit), False ignores it (exhaustive,
        the default); None leaves the mode the engine starts with (MM2GB_CHAIN_SKIP=keep|ignore, else exhaustive)."""
        L = lib()
        self.misc = misc if misc is not None else default_misc()
        self.config = config if config is not None else default_config()
        self.device = int(device)
        self._h = L.mm2gb_engine_create(C.byref(self.config), C.byref(self.misc), device)
        if not self._h:
            raise Mm2gbError(L.mm2gb_last_error().decode())
        if chain_skip is not None:
            self.set_chain_skip(chain_skip)

    def close(self):
        if getattr(self, "_h", None):
            lib().mm2gb_engine_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_misc(self, misc):
        _check(lib().mm2gb_engine_set_misc(self._h, C.byref(misc)))
        self.misc = misc

    def set_chain_skip(self, keep):
        """keep=True: later calls keep misc.max_skip in the chaining DP (the skip-limited walk); False: exhaustive whatever max_skip is."""
        _check(lib().mm2gb_engine_set_chain_skip(self._h, 1 if keep else 0))

    def last_score_form(self):
        """Form of the DP the last call ran: 0 exhaustive (k_score), 1 the skip-limited walk (k_skip_fill)."""
        return int(lib().mm2gb_engine_last_score_form(self._h))

    def last_score_mode(self):
        """Build of k_score that did the work of the last call's last micro-batch: 0 penalty table (LUT), 1 per-pair float penalties (FAST),
        2 every branch of comput_sc (GENERAL): the host's choice for the parameters combined with the device's flag word.  Waits for the engine."""
        m = int(lib().mm2gb_engine_last_score_mode(self._h))
        if m < 0:
            raise Mm2gbError(lib().mm2gb_last_error().decode())
        return m

    def band_groups(self):
        """Groups of 64 targets k_score's band pass swept in the last call: (wave path, team paths)."""
        out = (C.c_int64 * 2)()
        _check(lib().mm2gb_engine_band_groups(self._h, out))
        return int(out[0]), int(out[1])

    def sparse_chunks(self):
        """Chunks of the planner's sparse list (stretches of isolated anchors) that the score kernel scored in the last call."""
        L = lib()
        L.mm2gb_engine_sparse_chunks.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        n = C.c_int64()
        _check(L.mm2gb_engine_sparse_chunks(self._h, C.byref(n)))
        return int(n.value)

    def band_shape(self):
        """The band pass's shape as configured: the slab (0: off), the lag of each path and the mean window above which a chunk takes it."""
        L = lib()
        L.mm2gb_engine_band_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        out = (C.c_int * 6)()
        _check(L.mm2gb_engine_band_shape(self._h, out))
        return dict(zip(("slab", "lag_wave", "lag_team4", "lag_team8", "lag_wg", "min_window"), (int(v) for v in out)))

    def cu_count(self):
        """Compute units of the engine's device (mm2gb_engine_cu_count): what the kernels that cap their grids by it use."""
        L = lib()
        L.mm2gb_engine_cu_count.argtypes = [C.c_void_p]
        return int(L.mm2gb_engine_cu_count(self._h))

    def skip_stats(self):
        """Counters of the skip-limited walk's last micro-batch (engine made with MM2GB_SKIP_STATS=1): rounds of 64 candidates, max_ii search
        rounds, targets, the slowest chunk's ticks and anchors, the walk's span in ticks (100 MHz clock)."""
        L = lib()
        L.mm2gb_engine_skip_stats.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(6, dtype=np.int64)
        _check(L.mm2gb_engine_skip_stats(self._h, out.ctypes.data))
        keys = ("rounds", "rescan_rounds", "targets", "slowest_chunk_ticks", "slowest_chunk_anchors", "span_ticks")
        return {k: int(v) for k, v in zip(keys, out)}

    def gang_counts(self):
        """Of the last completed call: (chunks scored by a gang of workgroups, workgroups that started in a gang)."""
        c, h = C.c_int64(), C.c_int64()
        lib().mm2gb_engine_gang_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib().mm2gb_engine_gang_counts.restype = None
        lib().mm2gb_engine_gang_counts(self._h, C.byref(c), C.byref(h))
        return c.value, h.value

    def score(self, anchors, offsets):
        """Host buffers in, host buffers out.  anchors: (n,2) uint64; offsets: (R+1,) int64.
        Returns f int32[n], p int32[n] (distance back to the predecessor, 0 = none), stats dict."""
        a = np.ascontiguousarray(anchors, dtype=np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = int(off[-1])
        assert a.shape == (n, 2)
        f = np.empty(n, dtype=np.int32)
        p = np.empty(n, dtype=np.int32)
        st = Stats()
        _check(lib().mm2gb_score_host(self._h, len(off) - 1, off.ctypes.data, a.ctypes.data, f.ctypes.data, p.ctypes.data, C.byref(st)))
        return f, p, st.as_dict()

    def score_device(self, n_reads, d_offsets, d_anchors, n_anchors, d_f, d_p):
        """Raw device pointers (ints); asynchronous on the engine's stream."""
        _check(lib().mm2gb_score_device(self._h, n_reads, d_offsets, d_anchors, n_anchors, d_f, d_p))

    def sync(self):
        _check(lib().mm2gb_engine_sync(self._h))

    def stats(self):
        st = Stats()
        _check(lib().mm2gb_engine_stats(self._h, C.byref(st)))
        return st.as_dict()

    def stream(self):
        return lib().mm2gb_engine_stream(self._h)

    def chain(self, anchors, offsets, threads=1):
        """Full chaining of a batch: returns list of (u, a_out) per read plus stats."""
        a = np.ascontiguousarray(anchors, dtype=np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        R = len(off) - 1
        out = Chains()
        st = Stats()
        _check(lib().mm2gb_chain_host(self._h, R, off.ctypes.data, a.ctypes.data, threads, C.byref(out), C.byref(st)))
        return _take_chains(out, R), st.as_dict()


def _engine_chain_gpu(self, anchors, offsets):
    """Full chaining of a batch with backtrack + compaction on the device too (mm2gb_chain_gpu): list of (u, a_out) per read."""
    a = np.ascontiguousarray(anchors, dtype=np.uint64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    R = len(off) - 1
    out = Chains()
    st = Stats()
    _check(lib().mm2gb_chain_gpu(self._h, R, off.ctypes.data, a.ctypes.data, C.byref(out), C.byref(st)))
    return _take_chains(out, R), st.as_dict()


Engine.chain_gpu = _engine_chain_gpu


def default_rmq_param(**kw):
    """What post_chaining_helper passes to mg_lchain_rmq for map-ont defaults (map.c:450-451), max_chain_skip = infinity."""
    d = dict(max_dist=5000, max_dist_inner=1000, bw=20000, max_chn_skip=INT32_MAX, cap_rmq_size=100000, min_cnt=3, min_sc=40,
             chn_pen_gap=np.float32(0.8 * 0.01 * 15), chn_pen_skip=np.float32(0.0))
    d.update(kw)
    return RmqParam(**d)


def _engine_rmq_chain(self, anchors, offsets, prm):
    """RMQ re-chaining of a batch on the device (mm2gb_rmq_chain_gpu): list of (u, a_out) per read, n_tied per read, stats."""
    a = np.ascontiguousarray(anchors, dtype=np.uint64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    R = len(off) - 1
    out = Chains()
    st = Stats()
    tied = np.zeros(max(R, 1), dtype=np.int32)
    _check(lib().mm2gb_rmq_chain_gpu(self._h, C.byref(prm), R, off.ctypes.data, a.ctypes.data, C.byref(out), tied.ctypes.data, C.byref(st)))
    return _take_chains(out, R), tied[:R], st.as_dict()


Engine.rmq_chain = _engine_rmq_chain


class RmqDeal(C.Structure):
    _fields_ = [("n_device", C.c_int64), ("n_host_cost", C.c_int64), ("n_host_tie", C.c_int64), ("est_device_s", C.c_double), ("est_host_s", C.c_double),
                ("device_s", C.c_double), ("host_s", C.c_double), ("tie_s", C.c_double), ("total_s", C.c_double), ("device_kernel", C.c_int32), ("n_team", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _engine_rmq_chain_exact(self, anchors, offsets, prm, threads=4):
    """mm2gb_rmq_chain: device and host threads at the same time, exact for every read: list of (u, a_out) per read, where each read was
    done (0 device, 1 host by cost, 2 host after a tie), the deal."""
    L = lib()
    L.mm2gb_rmq_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    a = np.ascontiguousarray(anchors, dtype=np.uint64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    R = len(off) - 1
    out = Chains()
    where = np.zeros(max(R, 1), dtype=np.int32)
    deal = RmqDeal()
    _check(L.mm2gb_rmq_chain(self._h, C.byref(prm), R, off.ctypes.data, a.ctypes.data, int(threads), C.byref(out), where.ctypes.data, C.byref(deal)))
    return _take_chains(out, R), where[:R], deal.as_dict()


Engine.rmq_chain_exact = _engine_rmq_chain_exact


def rmq_chain_host(anchors, offsets, prm, threads=4):
    """mm2gb_rmq_chain_host: the same re-chaining on host threads (segment tree): list of (u, a_out) per read, n_tied per read."""
    L = lib()
    L.mm2gb_rmq_chain_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    a = np.ascontiguousarray(anchors, dtype=np.uint64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    R = len(off) - 1
    out = Chains()
    tied = np.zeros(max(R, 1), dtype=np.int32)
    _check(L.mm2gb_rmq_chain_host(C.byref(prm), R, off.ctypes.data, a.ctypes.data, int(threads), C.byref(out), tied.ctypes.data))
    return _take_chains(out, R), tied[:R]

REG_DTYPE = np.dtype([(k, "<i4") for k in "id cnt rid score qs qe rs re parent subsc as_ mlen blen n_sub score0".split()] +
                     [("flags", "<u4"), ("hash", "<u4"), ("div", "<f4")])      # mm2gb_reg_t


def _engine_sort_seeds(self, anchors, offsets):
    """mm2gb_sort_seeds_gpu: every read's anchors sorted by x the way radix_sort_128x leaves them; returns the sorted copy."""
    a = np.ascontiguousarray(anchors, dtype=np.uint64).copy()
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    _check(lib().mm2gb_sort_seeds_gpu(self._h, len(off) - 1, off.ctypes.data, a.ctypes.data))
    return a


def _engine_collect_seeds(self, flag, reads, ref_len=None, ref_rank=None):
    """mm2gb_collect_seeds_gpu.  reads: list of dicts with seeds (n,4) uint32, hits (uint64), qlen and optionally q_rank.
    Returns one sorted anchor array (m,2) uint64 per read."""
    R = len(reads)
    seed_off = np.zeros(R + 1, np.int64)
    seed_off[1:] = np.cumsum([len(r["seeds"]) for r in reads])
    seeds = np.ascontiguousarray(np.concatenate([np.asarray(r["seeds"], np.uint32).reshape(-1, 4) for r in reads]) if R else np.zeros((0, 4), np.uint32), dtype=np.uint32)
    hit_off = np.zeros(len(seeds) + 1, np.int64)
    np.cumsum(seeds[:, 0], out=hit_off[1:])
    hits = np.ascontiguousarray(np.concatenate([np.asarray(r["hits"], np.uint64) for r in reads]) if R else np.zeros(0, np.uint64), dtype=np.uint64)
    qlen = np.ascontiguousarray([r["qlen"] for r in reads], dtype=np.int32)
    have_rank = any("q_rank" in r for r in reads)
    q_rank = np.ascontiguousarray([r.get("q_rank", 0) for r in reads], dtype=np.int32) if have_rank else None
    rl = np.ascontiguousarray(ref_len, dtype=np.int32) if ref_len is not None else None
    rr = np.ascontiguousarray(ref_rank, dtype=np.int32) if ref_rank is not None else None
    n_ref = len(rl) if rl is not None else (len(rr) if rr is not None else 0)
    a_off = np.zeros(R + 1, np.int64)
    out = np.zeros((max(len(hits), 1), 2), np.uint64)
    _check(lib().mm2gb_collect_seeds_gpu(self._h, int(flag), R, seed_off.ctypes.data, seeds.ctypes.data, hit_off.ctypes.data, hits.ctypes.data, qlen.ctypes.data,
                                         q_rank.ctypes.data if q_rank is not None else None, n_ref, rl.ctypes.data if rl is not None else None,
                                         rr.ctypes.data if rr is not None else None, a_off.ctypes.data, out.ctypes.data))
    return [out[a_off[r]:a_off[r + 1]].copy() for r in range(R)]


def _engine_gen_regs(self, chains, qlen, hashes, is_qstrand=0):
    """mm2gb_gen_regs_gpu on a list of (u, a_out) per read: list of REG_DTYPE arrays."""
    R = len(chains)
    u_off = np.zeros(R + 1, np.int64); a_off = np.zeros(R + 1, np.int64)
    u_off[1:] = np.cumsum([len(u) for u, _ in chains]); a_off[1:] = np.cumsum([len(a) for _, a in chains])
    u_all = np.ascontiguousarray(np.concatenate([u for u, _ in chains]) if R else np.zeros(0, np.uint64), dtype=np.uint64)
    a_all = np.ascontiguousarray(np.concatenate([a for _, a in chains]) if R else np.zeros((0, 2), np.uint64), dtype=np.uint64)
    ch = Chains(u_off.ctypes.data_as(C.POINTER(C.c_int64)), u_all.ctypes.data_as(C.POINTER(C.c_uint64)), a_off.ctypes.data_as(C.POINTER(C.c_int64)), a_all.ctypes.data)
    ql = np.ascontiguousarray(qlen, dtype=np.int32); hs = np.ascontiguousarray(hashes, dtype=np.uint32)
    regs = np.zeros(int(u_off[-1]), dtype=REG_DTYPE)
    _check(lib().mm2gb_gen_regs_gpu(self._h, R, C.byref(ch), ql.ctypes.data, hs.ctypes.data, int(is_qstrand), regs.ctypes.data))
    return [regs[u_off[r]:u_off[r + 1]] for r in range(R)]


Engine.sort_seeds = _engine_sort_seeds
Engine.collect_seeds = _engine_collect_seeds


def collect_seeds_host(flag, reads, ref_len=None, ref_rank=None, threads=4):
    """mm2gb_collect_seeds_host: same arguments and results as Engine.collect_seeds, on host threads."""
    L = lib()
    L.mm2gb_collect_seeds_host.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    R = len(reads)
    seed_off = np.zeros(R + 1, np.int64)
    seed_off[1:] = np.cumsum([len(r["seeds"]) for r in reads])
    seeds = np.ascontiguousarray(np.concatenate([np.asarray(r["seeds"], np.uint32).reshape(-1, 4) for r in reads]) if R else np.zeros((0, 4), np.uint32), dtype=np.uint32)
    hit_off = np.zeros(len(seeds) + 1, np.int64)
    np.cumsum(seeds[:, 0], out=hit_off[1:])
    hits = np.ascontiguousarray(np.concatenate([np.asarray(r["hits"], np.uint64) for r in reads]) if R else np.zeros(0, np.uint64), dtype=np.uint64)
    qlen = np.ascontiguousarray([r["qlen"] for r in reads], dtype=np.int32)
    have_rank = any("q_rank" in r for r in reads)
    q_rank = np.ascontiguousarray([r.get("q_rank", 0) for r in reads], dtype=np.int32) if have_rank else None
    rl = np.ascontiguousarray(ref_len, dtype=np.int32) if ref_len is not None else None
    rr = np.ascontiguousarray(ref_rank, dtype=np.int32) if ref_rank is not None else None
    n_ref = len(rl) if rl is not None else (len(rr) if rr is not None else 0)
    a_off = np.zeros(R + 1, np.int64)
    out = np.zeros((max(len(hits), 1), 2), np.uint64)
    _check(L.mm2gb_collect_seeds_host(int(flag), R, seed_off.ctypes.data, seeds.ctypes.data, hit_off.ctypes.data, hits.ctypes.data, qlen.ctypes.data,
                                      q_rank.ctypes.data if q_rank is not None else None, n_ref, rl.ctypes.data if rl is not None else None,
                                      rr.ctypes.data if rr is not None else None, int(threads), a_off.ctypes.data, out.ctypes.data))
    return [out[a_off[r]:a_off[r + 1]].copy() for r in range(R)]
Engine.gen_regs = _engine_gen_regs


def _seed_arrays(reads, ref_len, ref_rank):
    """The arrays the seed collection calls take, from reads as Engine.collect_seeds takes them."""
    R = len(reads)
    seed_off = np.zeros(R + 1, np.int64)
    seed_off[1:] = np.cumsum([len(r["seeds"]) for r in reads])
    seeds = np.ascontiguousarray(np.concatenate([np.asarray(r["seeds"], np.uint32).reshape(-1, 4) for r in reads]) if R else np.zeros((0, 4), np.uint32), dtype=np.uint32)
    hit_off = np.zeros(len(seeds) + 1, np.int64)
    np.cumsum(seeds[:, 0], out=hit_off[1:])
    hits = np.ascontiguousarray(np.concatenate([np.asarray(r["hits"], np.uint64) for r in reads]) if R else np.zeros(0, np.uint64), dtype=np.uint64)
    qlen = np.ascontiguousarray([r["qlen"] for r in reads], dtype=np.int32)
    q_rank = np.ascontiguousarray([r.get("q_rank", 0) for r in reads], dtype=np.int32) if any("q_rank" in r for r in reads) else None
    rl = np.ascontiguousarray(ref_len, dtype=np.int32) if ref_len is not None else None
    rr = np.ascontiguousarray(ref_rank, dtype=np.int32) if ref_rank is not None else None
    n_ref = len(rl) if rl is not None else (len(rr) if rr is not None else 0)
    ptr = lambda a: a.ctypes.data if a is not None else None
    return R, seed_off, seeds, hit_off, hits, qlen, q_rank, rl, rr, n_ref, ptr


def _engine_collect_seeds_heap(self, flag, reads, ref_len=None, ref_rank=None):
    """mm2gb_collect_seeds_heap_gpu: Engine.collect_seeds with the anchors in the order collect_seed_hits_heap leaves them (minimap2 -x sr: MM_F_HEAP_SORT) -- forward
    strand first, each strand in ascending index position, equal positions in the reference heap's own order.  Returns (one (m,2) uint64 array per read, n_tied_reads):
    the reads with two equal positions, which the call does again with the host form."""
    R, seed_off, seeds, hit_off, hits, qlen, q_rank, rl, rr, n_ref, ptr = _seed_arrays(reads, ref_len, ref_rank)
    fn = lib().mm2gb_collect_seeds_heap_gpu
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(C.c_int64)]
    a_off = np.zeros(R + 1, np.int64)
    out = np.zeros((max(len(hits), 1), 2), np.uint64)
    n_tied = C.c_int64(0)
    _check(fn(self._h, int(flag), R, seed_off.ctypes.data, seeds.ctypes.data, hit_off.ctypes.data, hits.ctypes.data, qlen.ctypes.data, ptr(q_rank), n_ref, ptr(rl), ptr(rr),
              a_off.ctypes.data, out.ctypes.data, C.byref(n_tied)))
    return [out[a_off[r]:a_off[r + 1]].copy() for r in range(R)], int(n_tied.value)


Engine.collect_seeds_heap = _engine_collect_seeds_heap


def collect_seeds_heap_host(flag, reads, ref_len=None, ref_rank=None, threads=4):
    """mm2gb_collect_seeds_heap_host: the definition of Engine.collect_seeds_heap (map.c:229-293 with ksort.h's heap), on host threads; same arguments and results."""
    R, seed_off, seeds, hit_off, hits, qlen, q_rank, rl, rr, n_ref, ptr = _seed_arrays(reads, ref_len, ref_rank)
    fn = lib().mm2gb_collect_seeds_heap_host
    fn.argtypes = [C.c_int64, C.c_int64] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    a_off = np.zeros(R + 1, np.int64)
    out = np.zeros((max(len(hits), 1), 2), np.uint64)
    n_tied = C.c_int64(0)
    _check(fn(int(flag), R, seed_off.ctypes.data, seeds.ctypes.data, hit_off.ctypes.data, hits.ctypes.data, qlen.ctypes.data, ptr(q_rank), n_ref, ptr(rl), ptr(rr), int(threads),
              a_off.ctypes.data, out.ctypes.data, C.byref(n_tied)))
    return [out[a_off[r]:a_off[r + 1]].copy() for r in range(R)], int(n_tied.value)


# ---- base-level DP (mm2gb_ksw_extd2_host / _gpu): the dual-affine extension alignment of ksw2, batched ----
KSW_SCORE_ONLY, KSW_RIGHT, KSW_GENERIC_SC, KSW_APPROX_MAX, KSW_APPROX_DROP, KSW_EXTZ_ONLY, KSW_REV_CIGAR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x40, 0x80
KSW_NEG_INF = -0x40000000
KSW_FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "reach_end", "n_cigar")
KSW_JOB_DTYPE = np.dtype([("q_off", "<i8"), ("t_off", "<i8")] + [(k, "<i4") for k in "qlen tlen w zdrop end_bonus flag".split()])      # mm2gb_ksw_job_t
KSW_RES_DTYPE = np.dtype([(k, "<i4") for k in KSW_FIELDS + ("pad_",)] + [("cigar_off", "<i8")])                                         # mm2gb_ksw_res_t


class KswParam(C.Structure):
    """mm2gb_ksw_param_t: m residue codes (m - 1 the wildcard), the m x m matrix (row = target residue), the two gap pairs."""
    _fields_ = [("m", C.c_int8), ("mat", C.c_int8 * 25), ("q", C.c_int8), ("e", C.c_int8), ("q2", C.c_int8), ("e2", C.c_int8)]


def ksw_param(q=4, e=2, q2=24, e2=1, a=2, b=4, sc_ambi=1, mat=None, m=5):
    """The parameters of a batch; without mat, ksw_gen_simple_mat's matrix for match a, mismatch -b and wildcard -sc_ambi (align.c:9-21)."""
    p = KswParam()
    p.m, p.q, p.e, p.q2, p.e2 = int(m), int(q), int(e), int(q2), int(e2)
    if mat is None:
        mat = [[(a if i == j else -abs(b)) if i < m - 1 and j < m - 1 else -abs(sc_ambi) for j in range(m)] for i in range(m)]
    flat = np.asarray(mat, np.int8).reshape(-1)
    for k in range(min(len(flat), 25)):
        p.mat[k] = int(flat[k])
    return p


def ksw_jobs(pairs, w=-1, zdrop=-1, end_bonus=0, flag=0):
    """pairs: (query, target) or (query, target, dict of w / zdrop / end_bonus / flag for that job), sequences as uint8 codes.
    Returns the job records and the two concatenated sequence arrays the batch calls take."""
    jobs = np.zeros(len(pairs), KSW_JOB_DTYPE)
    qs = [np.asarray(p[0], np.uint8).reshape(-1) for p in pairs]
    ts = [np.asarray(p[1], np.uint8).reshape(-1) for p in pairs]
    jobs["qlen"] = [len(x) for x in qs]; jobs["tlen"] = [len(x) for x in ts]
    jobs["q_off"][1:] = np.cumsum(jobs["qlen"][:-1], dtype=np.int64); jobs["t_off"][1:] = np.cumsum(jobs["tlen"][:-1], dtype=np.int64)
    for name, dflt in (("w", w), ("zdrop", zdrop), ("end_bonus", end_bonus), ("flag", flag)):
        jobs[name] = [int(p[2].get(name, dflt)) if len(p) > 2 else int(dflt) for p in pairs]
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0, np.uint8), dtype=np.uint8)
    return jobs, cat(qs), cat(ts)


def _ksw_call(fn, head, param, jobs, queries, targets, tail, junc=()):
    """junc: () for the extd2 calls; for the exts2 calls (None,) or (array indexed like targets,)."""
    jobs = np.ascontiguousarray(jobs, dtype=KSW_JOB_DTYPE)
    queries = np.ascontiguousarray(queries, dtype=np.uint8); targets = np.ascontiguousarray(targets, dtype=np.uint8)
    junc = tuple(None if x is None else np.ascontiguousarray(x, dtype=np.uint8) for x in junc)
    for x in junc:
        if x is not None and len(x) != len(targets):
            raise Mm2gbError(f"junc has {len(x)} bytes, targets {len(targets)}: it is indexed like targets")
    res = np.zeros(len(jobs), KSW_RES_DTYPE)
    cig, total = C.c_void_p(), C.c_int64(0)
    fn.argtypes = [C.c_void_p] * len(head) + [C.POINTER(type(param)), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p] * len(junc) + [C.c_int] * len(tail) + \
                  [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    _check(fn(*head, C.byref(param), len(jobs), jobs.ctypes.data, queries.ctypes.data, targets.ctypes.data, *[None if x is None else x.ctypes.data for x in junc], *tail,
              res.ctypes.data, C.byref(cig), C.byref(total)))
    try:
        words = np.ctypeslib.as_array(C.cast(cig, C.POINTER(C.c_uint32)), shape=(total.value,)).copy() if total.value else np.zeros(0, np.uint32)
    finally:
        lib().mm2gb_free(cig)
    return res, words


def ksw_extd2_host_batch(param, jobs, queries, targets, threads=4):
    """mm2gb_ksw_extd2_host on packed arrays (ksw_jobs): the result records (KSW_RES_DTYPE) and the batch's CIGAR words."""
    return _ksw_call(lib().mm2gb_ksw_extd2_host, (), param, jobs, queries, targets, (int(threads),))


def _engine_ksw_extd2_batch(self, param, jobs, queries, targets):
    """mm2gb_ksw_extd2_gpu on packed arrays: as ksw_extd2_host_batch, on the device."""
    return _ksw_call(lib().mm2gb_ksw_extd2_gpu, (self._h,), param, jobs, queries, targets, ())


def _ksw_dicts(res, words):
    return [dict({k: int(r[k]) for k in KSW_FIELDS}, cigar=words[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])].copy()) for r in res]


def ksw_extd2_host(pairs, param=None, w=-1, zdrop=-1, end_bonus=0, flag=0, threads=4):
    """The extension DP for every (query, target) of pairs on host threads -- the definition.  One dict per job: the eleven fields of
    KSW_FIELDS and `cigar`, uint32 words len << 4 | op (0 M, 1 I, 2 D)."""
    return _ksw_dicts(*ksw_extd2_host_batch(param or ksw_param(), *ksw_jobs(pairs, w, zdrop, end_bonus, flag), threads=threads))


def _engine_ksw_extd2(self, pairs, param=None, w=-1, zdrop=-1, end_bonus=0, flag=0):
    """ksw_extd2_host's arguments and results, computed on the device (csrc/ksw_kernels.hip)."""
    return _ksw_dicts(*self.ksw_extd2_batch(param or ksw_param(), *ksw_jobs(pairs, w, zdrop, end_bonus, flag)))


def _engine_ksw_info(self):
    """The device form's seams and the last call's kernel times: dict with nt (threads per band class), band (widest rounded band of the
    first two classes), lds_max (largest image kept in LDS, bytes), ms_fill, ms_pack."""
    c = (C.c_int64 * 6)(); ms = (C.c_double * 2)()
    fn = lib().mm2gb_ksw_gpu_info
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _check(fn(self._h, c, ms))
    return dict(nt=list(c[0:3]), band=list(c[3:5]), lds_max=int(c[5]), ms_fill=ms[0], ms_pack=ms[1])


Engine.ksw_extd2 = _engine_ksw_extd2
Engine.ksw_extd2_batch = _engine_ksw_extd2_batch


# ---- single-affine DP (mm2gb_ksw_extz2_host / _gpu): ksw2's ksw_extz2_sse, what mm_align_pair runs at q == q2 && e == e2.  The calls mirror
#      the extd2 ones; of the parameters only m, mat, q and e are read ----
def ksw_extz2_host_batch(param, jobs, queries, targets, threads=4):
    """mm2gb_ksw_extz2_host on packed arrays (ksw_jobs): the result records (KSW_RES_DTYPE) and the batch's CIGAR words."""
    return _ksw_call(lib().mm2gb_ksw_extz2_host, (), param, jobs, queries, targets, (int(threads),))


def _engine_ksw_extz2_batch(self, param, jobs, queries, targets):
    """mm2gb_ksw_extz2_gpu on packed arrays: as ksw_extz2_host_batch, on the device."""
    return _ksw_call(lib().mm2gb_ksw_extz2_gpu, (self._h,), param, jobs, queries, targets, ())


def ksw_extz2_host(pairs, param=None, w=-1, zdrop=-1, end_bonus=0, flag=0, threads=4):
    """The single-affine extension DP for every (query, target) of pairs on host threads -- the definition.  Arguments and results are
    ksw_extd2_host's; param's q2 and e2 are not read."""
    return _ksw_dicts(*ksw_extz2_host_batch(param or ksw_param(), *ksw_jobs(pairs, w, zdrop, end_bonus, flag), threads=threads))


def _engine_ksw_extz2(self, pairs, param=None, w=-1, zdrop=-1, end_bonus=0, flag=0):
    """ksw_extz2_host's arguments and results, computed on the device (csrc/ksw_kernels.hip)."""
    return _ksw_dicts(*self.ksw_extz2_batch(param or ksw_param(), *ksw_jobs(pairs, w, zdrop, end_bonus, flag)))


Engine.ksw_extz2 = _engine_ksw_extz2
Engine.ksw_extz2_batch = _engine_ksw_extz2_batch
def _engine_ksw_class_jobs(self):
    """mm2gb_ksw_gpu_class_jobs: the DP jobs launched on this engine so far with their image (in LDS, in global memory)."""
    c = (C.c_int64 * 2)()
    fn = lib().mm2gb_ksw_gpu_class_jobs
    fn.argtypes = [C.c_void_p, C.c_void_p]
    _check(fn(self._h, c))
    return int(c[0]), int(c[1])


Engine.ksw_info = _engine_ksw_info
Engine.ksw_class_jobs = _engine_ksw_class_jobs


# ---- splice-aware DP (mm2gb_ksw_exts2_host / _gpu): ksw2's ksw_exts2_sse, batched.  Jobs, records and words as above; w and end_bonus are not
#      read, reach_end is always 0, and words may carry operation 3 (N). ----
KSW_SPLICE_FOR, KSW_SPLICE_REV, KSW_SPLICE_FLANK = 0x100, 0x200, 0x400


class KswSpliceParam(C.Structure):
    """mm2gb_ksw_splice_param_t: m, the m x m matrix, the short gap (q, e), the long gap's opening q2, the cost of a non-canonical splice site
    and the bonus of an annotated one."""
    _fields_ = [("m", C.c_int8), ("mat", C.c_int8 * 25), ("q", C.c_int8), ("e", C.c_int8), ("q2", C.c_int8), ("noncan", C.c_int8), ("junc_bonus", C.c_int8)]


def ksw_splice_param(a=1, b=2, sc_ambi=1, q=2, e=1, q2=32, noncan=9, junc_bonus=9, mat=None, m=5):
    """The parameters of a batch; the defaults are the `splice` preset's.  mat as in ksw_param."""
    p = KswSpliceParam()
    p.m, p.q, p.e, p.q2, p.noncan, p.junc_bonus = int(m), int(q), int(e), int(q2), int(noncan), int(junc_bonus)
    p.mat[:] = ksw_param(a=a, b=b, sc_ambi=sc_ambi, mat=mat, m=m).mat[:]
    return p


def ksw_splice_jobs(pairs, zdrop=-1, flag=0):
    """ksw_jobs for the exts2 calls: a pair's dict may also carry `junc`, one byte per target residue (bits 1 / 2 / 4 / 8).  Returns the job
    records, the two sequence arrays and the annotation array (None when no pair has one; zeros for the pairs without)."""
    jobs, queries, targets = ksw_jobs(pairs, -1, zdrop, 0, flag)
    if not any(len(p) > 2 and p[2].get("junc") is not None for p in pairs):
        return jobs, queries, targets, None
    junc = np.zeros(len(targets), np.uint8)
    for p, j in zip(pairs, jobs):
        if len(p) > 2 and p[2].get("junc") is not None:
            junc[int(j["t_off"]):int(j["t_off"]) + int(j["tlen"])] = np.asarray(p[2]["junc"], np.uint8).reshape(-1)
    return jobs, queries, targets, junc


def ksw_exts2_host_batch(param, jobs, queries, targets, junc=None, threads=4):
    """mm2gb_ksw_exts2_host on packed arrays (ksw_splice_jobs): the result records (KSW_RES_DTYPE) and the batch's CIGAR words."""
    return _ksw_call(lib().mm2gb_ksw_exts2_host, (), param, jobs, queries, targets, (int(threads),), junc=(junc,))


def _engine_ksw_exts2_batch(self, param, jobs, queries, targets, junc=None):
    """mm2gb_ksw_exts2_gpu on packed arrays: as ksw_exts2_host_batch, on the device."""
    return _ksw_call(lib().mm2gb_ksw_exts2_gpu, (self._h,), param, jobs, queries, targets, (), junc=(junc,))


def ksw_exts2_host(pairs, param=None, zdrop=-1, flag=0, threads=4):
    """The splice-aware DP for every (query, target[, dict of zdrop / flag / junc]) of pairs on host threads -- the definition.  One dict per
    job, as ksw_extd2_host gives; words len << 4 | op (0 M, 1 I, 2 D, 3 N)."""
    return _ksw_dicts(*ksw_exts2_host_batch(param or ksw_splice_param(), *ksw_splice_jobs(pairs, zdrop, flag), threads=threads))


def _engine_ksw_exts2(self, pairs, param=None, zdrop=-1, flag=0):
    """ksw_exts2_host's arguments and results, computed on the device (csrc/ksw_kernels.hip)."""
    return _ksw_dicts(*self.ksw_exts2_batch(param or ksw_splice_param(), *ksw_splice_jobs(pairs, zdrop, flag)))


Engine.ksw_exts2 = _engine_ksw_exts2
Engine.ksw_exts2_batch = _engine_ksw_exts2_batch


# ---- base-level alignment of hits (mm2gb_align_regs_host / _gpu): mm_align_skeleton for a batch of reads ----
F_SPLICE, F_SR, F_FOR_ONLY, F_REV_ONLY, F_EQX, F_NO_END_FLT, F_QSTRAND, F_NO_INV = 0x080, 0x1000, 0x100000, 0x200000, 0x4000000, 0x10000000, 0x100000000, 0x200000000
ALN_DTYPE = np.dtype([(k, "<i4") for k in "dp_score dp_max dp_max2 n_ambi trans_strand n_cigar".split()] + [("cigar_off", "<i8")])      # mm2gb_aln_t
ALN_COUNTS = ("gap_skipped", "fill_one_pass", "fill_two_pass", "split", "reads_3_rounds", "split_refused", "inv", "left_end", "left_short", "right_end", "right_short",
              "left_at_0", "rev_chain", "seam_merged", "lead_gap_cut", "filtered", "dp_max_rewritten", "over_sw_mat", "rounds", "hpc_moved", "inv_probe_hit",
              "jobs", "cells", "cells_discarded")
ALN_STAGES = ("upload", "planning", "gather", "first_pass", "test", "second_pass", "copies_back", "stitching")


class AlignOpt(C.Structure):
    """mm2gb_align_opt_t: the fields of mm_mapopt_t that mm_align_skeleton and what it calls read."""
    _fields_ = [("flag", C.c_int64), ("max_sw_mat", C.c_int64)] + [(k, C.c_int32) for k in "a b q e q2 e2 sc_ambi zdrop zdrop_inv end_bonus min_dp_max min_ksw_len bw bw_long max_gap min_cnt min_chain_score rank_min_len".split()] + \
               [("max_clip_ratio", C.c_float), ("rank_frac", C.c_float)]


class _AlignOut(C.Structure):
    _fields_ = [("n_regs", C.c_int64), ("n_cigar", C.c_int64), ("reg_off", C.c_void_p), ("regs", C.c_void_p), ("aln", C.c_void_p), ("cigar", C.c_void_p),
                ("counts", C.c_int64 * len(ALN_COUNTS)), ("seconds", C.c_double * 8)]


def align_opt(preset="map-ont", **kw):
    """mm2gb_align_opt_init for "map-ont", "map-pb", "map-hifi" / "map-ccs", "asm5", "asm10" or "asm20", then keyword overrides."""
    o = AlignOpt()
    fn = lib().mm2gb_align_opt_init
    fn.argtypes = [C.POINTER(AlignOpt), C.c_char_p]
    _check(fn(C.byref(o), preset.encode()))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise Mm2gbError(f"mm2gb_align_opt_t has no field {k!r}")
        setattr(o, k, v)
    return o


def cigar_string(words):
    """CIGAR words (len << 4 | op) as text, MM_CIGAR_STR's letters."""
    return "".join(f"{int(w) >> 4}{'MIDNSHP=XB'[int(w) & 0xf]}" for w in words)


def _align_call(fn, head, opt, k, hpc, refs, reads, regs, anchors, tail, opt_type=None, after=()):
    """reads: list of bytes; regs / anchors: one REG_DTYPE array / (n,2) uint64 array per read.  Returns per read (regs, aln, words) with
    aln.cigar_off counted within the read's words, and dict(counts=..., seconds=...)."""
    refs = [bytes(s) for s in refs]; reads = [bytes(s) for s in reads]
    R = len(reads)
    ref_arr = (C.c_char_p * max(len(refs), 1))(*refs); read_arr = (C.c_char_p * max(R, 1))(*reads)
    ref_len = np.ascontiguousarray([len(s) for s in refs], dtype=np.int32); read_len = np.ascontiguousarray([len(s) for s in reads], dtype=np.int32)
    reg_off = np.zeros(R + 1, np.int64); a_off = np.zeros(R + 1, np.int64)
    reg_off[1:] = np.cumsum([len(x) for x in regs]); a_off[1:] = np.cumsum([len(x) for x in anchors])
    reg_all = np.ascontiguousarray(np.concatenate([np.asarray(x, REG_DTYPE) for x in regs]) if R else np.zeros(0, REG_DTYPE), dtype=REG_DTYPE)
    a_all = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint64).reshape(-1, 2) for x in anchors]) if R else np.zeros((0, 2), np.uint64), dtype=np.uint64)
    out = _AlignOut()
    fn.argtypes = [C.c_void_p] * len(head) + [C.POINTER(opt_type or AlignOpt), C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * len(tail) + [C.POINTER(_AlignOut)] + [C.c_void_p] * len(after)
    _check(fn(*head, C.byref(opt), int(k), I_HPC if hpc else 0, len(refs), ref_arr, ref_len.ctypes.data, R, read_arr, read_len.ctypes.data,
              reg_off.ctypes.data, reg_all.ctypes.data, a_off.ctypes.data, a_all.ctypes.data, *tail, C.byref(out), *[C.addressof(x) for x in after]))
    try:
        off = _take(out.reg_off, R + 1, np.int64)
        rg = _take(out.regs, out.n_regs, REG_DTYPE); al = _take(out.aln, out.n_regs, ALN_DTYPE); words = _take(out.cigar, out.n_cigar, np.uint32)
    finally:
        free = lib().mm2gb_align_out_free
        free.argtypes = [C.POINTER(_AlignOut)]; free.restype = None
        free(C.byref(out))
    res = []
    for r in range(R):
        a = al[off[r]:off[r + 1]].copy()
        have = a["cigar_off"] >= 0
        lo = int(a["cigar_off"][have].min()) if have.any() else 0
        hi = int((a["cigar_off"] + a["n_cigar"])[have].max()) if have.any() else 0
        a["cigar_off"][have] -= lo
        res.append((rg[off[r]:off[r + 1]].copy(), a, words[lo:hi].copy()))
    return res, dict(counts=dict(zip(ALN_COUNTS, (int(x) for x in out.counts))), seconds=dict(zip(ALN_STAGES, (float(x) for x in out.seconds))))


def align_regs_host(opt, k, hpc, refs, reads, regs, anchors, threads=4):
    """mm2gb_align_regs_host: mm_align_skeleton for every read of a batch on host threads -- the definition (see _align_call)."""
    return _align_call(lib().mm2gb_align_regs_host, (), opt, k, hpc, refs, reads, regs, anchors, (int(threads),))


def _engine_align_regs(self, opt, k, hpc, refs, reads, regs, anchors):
    """mm2gb_align_regs_gpu: align_regs_host's arguments and results, the DP and its sequences on the device (csrc/align_kernels.hip)."""
    return _align_call(lib().mm2gb_align_regs_gpu, (self._h,), opt, k, hpc, refs, reads, regs, anchors, ())


Engine.align_regs = _engine_align_regs


# ---- the same calls for q == q2 && e == e2 (minimap2 -O4 -E2), where every stretch goes through the single-affine DP (ksw_extz2) ----
def align_regs_extz_host(opt, k, hpc, refs, reads, regs, anchors, threads=4):
    """mm2gb_align_regs_extz_host: align_regs_host's arguments and results for an option set with q == q2 and e == e2
    (align_opt("map-ont", q2=4, e2=2)), which align_regs_host refuses -- the definition."""
    return _align_call(lib().mm2gb_align_regs_extz_host, (), opt, k, hpc, refs, reads, regs, anchors, (int(threads),))


def _engine_align_regs_extz(self, opt, k, hpc, refs, reads, regs, anchors):
    """mm2gb_align_regs_extz_gpu: align_regs_extz_host's arguments and results, the DP and its sequences on the device."""
    return _align_call(lib().mm2gb_align_regs_extz_gpu, (self._h,), opt, k, hpc, refs, reads, regs, anchors, ())


Engine.align_regs_extz = _engine_align_regs_extz


# ---- spliced alignment of hits (mm2gb_align_regs_splice_host / _gpu): mm_align_skeleton under MM_F_SPLICE; the calls above keep refusing it ----
F_SPLICE_FOR, F_SPLICE_REV, F_SPLICE_FLANK = 0x100, 0x200, 0x40000
SPLICE_COUNTS = ("trial_for_won", "trial_rev_won", "trial_tie_kept_0", "trial_tie_kept_1", "end_flt_head", "end_flt_tail", "end_flt_probe_kept", "left_ext_intron",
                 "right_ext_intron", "fill_intron", "fill_two_pass", "split", "tail_other_strand", "n_seam_merged", "noncanonical_intron", "single_trial", "rev_chain",
                 "over_sw_mat")


class AlignSpliceOpt(C.Structure):
    """mm2gb_align_splice_opt_t: mm2gb_align_opt_t and the four numbers only the spliced form reads."""
    _fields_ = [("base", AlignOpt)] + [(k, C.c_int32) for k in "noncan junc_bonus anchor_ext_len anchor_ext_shift".split()]


def align_splice_opt(preset="splice", **kw):
    """mm2gb_align_splice_opt_init for "splice", "cdna" or "splice:hq", then keyword overrides (a field of either record by its name)."""
    o = AlignSpliceOpt()
    fn = lib().mm2gb_align_splice_opt_init
    fn.argtypes = [C.POINTER(AlignSpliceOpt), C.c_char_p]
    _check(fn(C.byref(o), preset.encode()))
    own = {k for k, _ in AlignSpliceOpt._fields_[1:]}
    for k, v in kw.items():
        if k in own:
            setattr(o, k, v)
        elif hasattr(o.base, k):
            setattr(o.base, k, v)
        else:
            raise Mm2gbError(f"mm2gb_align_splice_opt_t has no field {k!r}")
    return o


def _align_splice_call(fn, head, opt, k, hpc, refs, reads, regs, anchors, tail):
    if not isinstance(opt, AlignSpliceOpt):
        raise Mm2gbError("the spliced alignment calls take an AlignSpliceOpt (align_splice_opt())")
    sc = (C.c_int64 * len(SPLICE_COUNTS))()
    res, info = _align_call(fn, head, opt, k, hpc, refs, reads, regs, anchors, tail, opt_type=AlignSpliceOpt, after=(sc,))
    info["splice_counts"] = dict(zip(SPLICE_COUNTS, (int(x) for x in sc)))
    return res, info


def align_regs_splice_host(opt, k, hpc, refs, reads, regs, anchors, threads=4):
    """mm2gb_align_regs_splice_host: align_regs_host's arguments and results for spliced reads, with info["splice_counts"] (the paths met)."""
    return _align_splice_call(lib().mm2gb_align_regs_splice_host, (), opt, k, hpc, refs, reads, regs, anchors, (int(threads),))


def _engine_align_regs_splice(self, opt, k, hpc, refs, reads, regs, anchors):
    """mm2gb_align_regs_splice_gpu: align_regs_splice_host's arguments and results, the DP and its sequences on the device."""
    return _align_splice_call(lib().mm2gb_align_regs_splice_gpu, (self._h,), opt, k, hpc, refs, reads, regs, anchors, ())


Engine.align_regs_splice = _engine_align_regs_splice


# ---- alignment of hits under MM_F_SR (mm2gb_align_regs_sr_host / _gpu): mm_align1's is_sr branches; the calls above keep refusing MM_F_SR ----
SR_COUNTS = ("fill_ungapped", "fill_rerun", "stretch_short")


def align_sr_opt(**kw):
    """mm2gb_align_sr_opt_init (options.c:133-150: a 2, b 8, q 12, e 2, q2 24, e2 1, zdrop = zdrop_inv = 100, end_bonus 10, min_dp_max 40, ...), then keyword overrides."""
    o = AlignOpt()
    fn = lib().mm2gb_align_sr_opt_init
    fn.argtypes = [C.POINTER(AlignOpt)]
    fn.restype = None
    fn(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise Mm2gbError(f"mm2gb_align_opt_t has no field {k!r}")
        setattr(o, k, v)
    return o


def _align_sr_call(fn, head, opt, k, hpc, refs, reads, regs, anchors, tail):
    sc = (C.c_int64 * len(SR_COUNTS))()
    res, info = _align_call(fn, head, opt, k, hpc, refs, reads, regs, anchors, tail, after=(sc,))
    info["sr_counts"] = dict(zip(SR_COUNTS, (int(x) for x in sc)))
    return res, info


def align_regs_sr_host(opt, k, hpc, refs, reads, regs, anchors, threads=4):
    """mm2gb_align_regs_sr_host: align_regs_host's arguments and results for short reads (opt: align_sr_opt()), with info["sr_counts"] -- the definition."""
    return _align_sr_call(lib().mm2gb_align_regs_sr_host, (), opt, k, hpc, refs, reads, regs, anchors, (int(threads),))


def _engine_align_regs_sr(self, opt, k, hpc, refs, reads, regs, anchors):
    """mm2gb_align_regs_sr_gpu: align_regs_sr_host's arguments and results; the ungapped first pass of every fill in k_al_ungapped, the DPs on the device."""
    return _align_sr_call(lib().mm2gb_align_regs_sr_gpu, (self._h,), opt, k, hpc, refs, reads, regs, anchors, ())


Engine.align_regs_sr = _engine_align_regs_sr


# ---- the text of a PAF line's alignment tags (mm2gb_aln_text_host / _gpu): cg:Z, cs:Z, MD:Z for a batch of records ----
TEXT_CG, TEXT_CS, TEXT_CS_LONG, TEXT_MD = 0x1, 0x2, 0x4, 0x8


def flatten_aligned(res):
    """What align_regs_host / Engine.align_regs return per read, as aln_text_* takes it: (regs, read_of_reg, aln, cigar), flat, with
    aln.cigar_off counted in cigar."""
    regs = np.concatenate([x[0] for x in res]) if res else np.zeros(0, REG_DTYPE)
    aln = np.concatenate([x[1] for x in res]).copy() if res else np.zeros(0, ALN_DTYPE)
    cigar = np.concatenate([x[2] for x in res]) if res else np.zeros(0, np.uint32)
    read_of = np.concatenate([np.full(len(x[0]), r, np.int32) for r, x in enumerate(res)]) if res else np.zeros(0, np.int32)
    base = np.concatenate([np.full(len(x[0]), b, np.int64) for x, b in zip(res, np.cumsum([0] + [len(x[2]) for x in res[:-1]]))]) if res else np.zeros(0, np.int64)
    have = aln["cigar_off"] >= 0
    aln["cigar_off"][have] += base[have]
    return regs, read_of, aln, cigar


def _aln_text_call(fn, head, what, refs, reads, regs, read_of_reg, aln, cigar, tail):
    refs = [bytes(s) for s in refs]; reads = [bytes(s) for s in reads]
    ref_arr = (C.c_char_p * max(len(refs), 1))(*refs); read_arr = (C.c_char_p * max(len(reads), 1))(*reads)
    ref_len = np.ascontiguousarray([len(s) for s in refs], dtype=np.int32); read_len = np.ascontiguousarray([len(s) for s in reads], dtype=np.int32)
    regs = np.ascontiguousarray(regs, dtype=REG_DTYPE); aln = np.ascontiguousarray(aln, dtype=ALN_DTYPE)
    read_of_reg = np.ascontiguousarray(read_of_reg, dtype=np.int32); cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    if not len(regs) == len(aln) == len(read_of_reg):
        raise Mm2gbError("aln_text: regs, read_of_reg and aln must have one entry per record")
    have = aln["cigar_off"] >= 0
    if have.any() and (int((aln["cigar_off"] + aln["n_cigar"])[have].max()) > len(cigar) or int(aln["n_cigar"][have].min()) < 0):
        raise Mm2gbError("aln_text: a record's CIGAR words lie outside cigar")
    off, text = C.c_void_p(0), C.c_void_p(0)
    fn.argtypes = [C.c_void_p] * len(head) + [C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p] + [C.c_int] * len(tail) + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    _check(fn(*head, int(what), len(refs), ref_arr, ref_len.ctypes.data, len(reads), read_arr, read_len.ctypes.data, len(regs), regs.ctypes.data, read_of_reg.ctypes.data,
              aln.ctypes.data, cigar.ctypes.data, *tail, C.byref(off), C.byref(text)))
    try:
        o = _take(off.value, len(regs) + 1, np.int64)
        return o, C.string_at(text.value, int(o[-1]))
    finally:
        lib().mm2gb_free(off); lib().mm2gb_free(text)


def aln_text_host(what, refs, reads, regs, read_of_reg, aln, cigar, threads=4):
    """mm2gb_aln_text_host: what mm_write_paf3 appends after rl:i for every record -- cg:Z (TEXT_CG), cs:Z (TEXT_CS, with TEXT_CS_LONG the long
    form) or MD:Z (TEXT_MD) -- the definition.  regs / aln: REG_DTYPE / ALN_DTYPE arrays, one entry per record, aln.cigar_off counted in cigar;
    read_of_reg: the read of every record (flatten_aligned makes all four from an alignment call's result).  Returns (offsets, bytes): record
    i's text is bytes[offsets[i]:offsets[i + 1]]."""
    return _aln_text_call(lib().mm2gb_aln_text_host, (), what, refs, reads, regs, read_of_reg, aln, cigar, (int(threads),))


def _engine_aln_text(self, what, refs, reads, regs, read_of_reg, aln, cigar):
    """mm2gb_aln_text_gpu: aln_text_host's arguments and results, every column on the device (csrc/aln_text_kernels.hip)."""
    return _aln_text_call(lib().mm2gb_aln_text_gpu, (self._h,), what, refs, reads, regs, read_of_reg, aln, cigar, ())


def _engine_aln_text_info(self):
    """The device form's seams and the last call's seconds: dict with slice (columns per slice), wg (threads of a workgroup), s_upload (residues), s_prepare (the host's pass over the words), s_kernels (words up and kernels), s_back."""
    c = (C.c_int64 * 2)(); s = (C.c_double * 4)()
    fn = lib().mm2gb_aln_text_gpu_info
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _check(fn(self._h, c, s))
    return dict(slice=int(c[0]), wg=int(c[1]), s_upload=s[0], s_prepare=s[1], s_kernels=s[2], s_back=s[3])


def aln_text_splice_host(what, refs, reads, regs, read_of_reg, aln, cigar, threads=4):
    """mm2gb_aln_text_splice_host: aln_text_host for records of the spliced alignment calls: N words are taken (cg:Z `N`, cs:Z `~gt123ag`, MD:Z nothing)."""
    return _aln_text_call(lib().mm2gb_aln_text_splice_host, (), what, refs, reads, regs, read_of_reg, aln, cigar, (int(threads),))


def _engine_aln_text_splice(self, what, refs, reads, regs, read_of_reg, aln, cigar):
    """mm2gb_aln_text_splice_gpu: aln_text_splice_host's arguments and results, every column on the device; an N word is one column."""
    return _aln_text_call(lib().mm2gb_aln_text_splice_gpu, (self._h,), what, refs, reads, regs, read_of_reg, aln, cigar, ())


Engine.aln_text = _engine_aln_text
Engine.aln_text_splice = _engine_aln_text_splice
Engine.aln_text_info = _engine_aln_text_info


# ---- = / X CIGARs (mm2gb_cigar_eqx_host / _gpu; minimap2 --eqx): mm_update_cigar_eqx for a batch of records ----
def _cigar_eqx_call(fn, head, refs, reads, regs, read_of_reg, aln, cigar, tail):
    refs = [bytes(s) for s in refs]; reads = [bytes(s) for s in reads]
    ref_arr = (C.c_char_p * max(len(refs), 1))(*refs); read_arr = (C.c_char_p * max(len(reads), 1))(*reads)
    ref_len = np.ascontiguousarray([len(s) for s in refs], dtype=np.int32); read_len = np.ascontiguousarray([len(s) for s in reads], dtype=np.int32)
    regs = np.ascontiguousarray(regs, dtype=REG_DTYPE); aln = np.ascontiguousarray(aln, dtype=ALN_DTYPE)
    read_of_reg = np.ascontiguousarray(read_of_reg, dtype=np.int32); cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    if not len(regs) == len(aln) == len(read_of_reg):
        raise Mm2gbError("cigar_eqx: regs, read_of_reg and aln must have one entry per record")
    have = aln["cigar_off"] >= 0
    if have.any() and (int((aln["cigar_off"] + aln["n_cigar"])[have].max()) > len(cigar) or int(aln["n_cigar"][have].min()) < 0):
        raise Mm2gbError("cigar_eqx: a record's CIGAR words lie outside cigar")
    a_out, w_out = C.c_void_p(0), C.c_void_p(0)
    fn.argtypes = [C.c_void_p] * len(head) + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p] + [C.c_int] * len(tail) + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    _check(fn(*head, len(refs), ref_arr, ref_len.ctypes.data, len(reads), read_arr, read_len.ctypes.data, len(regs), regs.ctypes.data, read_of_reg.ctypes.data,
              aln.ctypes.data, cigar.ctypes.data, *tail, C.byref(a_out), C.byref(w_out)))
    try:
        a = _take(a_out.value, len(regs), ALN_DTYPE)
        have = a["cigar_off"] >= 0
        n = int((a["cigar_off"] + a["n_cigar"])[have].max()) if have.any() else 0
        return a, _take(w_out.value, n, np.uint32)
    finally:
        lib().mm2gb_free(a_out); lib().mm2gb_free(w_out)


def cigar_eqx_host(refs, reads, regs, read_of_reg, aln, cigar, threads=4):
    """mm2gb_cigar_eqx_host: mm_update_cigar_eqx (minimap2 --eqx) on finished records -- every M word as runs of = (7) and X (8); I, D and N words
    copied -- the definition.  Arguments as aln_text_host's.  Returns (aln, cigar): aln with cigar_off / n_cigar of the new words, and the words;
    the input is untouched."""
    return _cigar_eqx_call(lib().mm2gb_cigar_eqx_host, (), refs, reads, regs, read_of_reg, aln, cigar, (int(threads),))


def _engine_cigar_eqx(self, refs, reads, regs, read_of_reg, aln, cigar):
    """mm2gb_cigar_eqx_gpu: cigar_eqx_host's arguments and results, every column on the device (csrc/eqx_kernels.hip)."""
    return _cigar_eqx_call(lib().mm2gb_cigar_eqx_gpu, (self._h,), refs, reads, regs, read_of_reg, aln, cigar, ())


def _engine_cigar_eqx_info(self):
    """As aln_text_info, for the last Engine.cigar_eqx call."""
    c = (C.c_int64 * 2)(); s = (C.c_double * 4)()
    fn = lib().mm2gb_cigar_eqx_gpu_info
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _check(fn(self._h, c, s))
    return dict(slice=int(c[0]), wg=int(c[1]), s_upload=s[0], s_prepare=s[1], s_kernels=s[2], s_back=s[3])


Engine.cigar_eqx = _engine_cigar_eqx
Engine.cigar_eqx_info = _engine_cigar_eqx_info


def _take_chains(out, R):
    """Copy a mm2gb_chains_t into per-read (u, a_out) arrays and release it."""
    try:
        u_off = np.ctypeslib.as_array(out.u_off, shape=(R + 1,)).copy()
        a_off = np.ctypeslib.as_array(out.a_off, shape=(R + 1,)).copy()
        u_all = np.ctypeslib.as_array(out.u, shape=(int(u_off[-1]),)).copy() if u_off[-1] else np.zeros(0, np.uint64)
        a_all = (np.ctypeslib.as_array(C.cast(out.a, C.POINTER(C.c_uint64)), shape=(int(a_off[-1]), 2)).copy()
                 if a_off[-1] else np.zeros((0, 2), np.uint64))
    finally:
        lib().mm2gb_chains_free(C.byref(out))
    return [(u_all[u_off[r]:u_off[r + 1]], a_all[a_off[r]:a_off[r + 1]]) for r in range(R)]


class Pool:
    """Several engines in one process (mm2gb_pool_t): reads are dealt to the devices as contiguous runs with about the same
    number of anchors, nothing is exchanged between devices.  devices=None: every visible GPU; ids may repeat."""

    def __init__(self, devices=None, misc=None, config=None):
        L = lib()
        self.misc = misc if misc is not None else default_misc()
        self.config = config if config is not None else default_config()
        ids = np.ascontiguousarray(devices, dtype=np.int32) if devices is not None else None
        self._h = L.mm2gb_pool_create(C.byref(self.config), C.byref(self.misc), 0 if ids is None else len(ids),
                                      None if ids is None else ids.ctypes.data)
        if not self._h:
            raise Mm2gbError(L.mm2gb_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().mm2gb_pool_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return lib().mm2gb_pool_size(self._h)

    def devices(self):
        return [lib().mm2gb_pool_device(self._h, k) for k in range(len(self))]

    def set_misc(self, misc):
        _check(lib().mm2gb_pool_set_misc(self._h, C.byref(misc)))
        self.misc = misc

    def score(self, anchors, offsets):
        """Like Engine.score; also returns first_read_of_device (len(pool)+1,) = how the reads were dealt."""
        a = np.ascontiguousarray(anchors, dtype=np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = int(off[-1])
        assert a.shape == (n, 2)
        f = np.empty(n, dtype=np.int32)
        p = np.empty(n, dtype=np.int32)
        first = np.zeros(len(self) + 1, dtype=np.int64)
        st = Stats()
        _check(lib().mm2gb_pool_score_host(self._h, len(off) - 1, off.ctypes.data, a.ctypes.data, f.ctypes.data, p.ctypes.data,
                                           C.byref(st), first.ctypes.data))
        return f, p, st.as_dict(), first

    def chain(self, anchors, offsets, threads=1):
        a = np.ascontiguousarray(anchors, dtype=np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        R = len(off) - 1
        out = Chains()
        st = Stats()
        _check(lib().mm2gb_pool_chain_host(self._h, R, off.ctypes.data, a.ctypes.data, threads, C.byref(out), C.byref(st)))
        return _take_chains(out, R), st.as_dict()


def plan_batches(n_anchors, max_total_n, max_read, min_n):
    """The batcher's grouping rule alone (no GPU): (number of batches, batch id per read, lane per read)."""
    n = np.ascontiguousarray(n_anchors, dtype=np.int64)
    batch = np.empty(len(n), dtype=np.int32)
    lane = np.empty(len(n), dtype=np.int32)
    nb = lib().mm2gb_plan_batches(len(n), n.ctypes.data, max_total_n, max_read, min_n, batch.ctypes.data, lane.ctypes.data)
    if nb < 0:
        raise Mm2gbError(lib().mm2gb_last_error().decode())
    return int(nb), batch, lane


class Batcher:
    """mm2gb_batcher_t: feed reads one at a time, get every read's chains back (dict read_id -> (u, a_out))."""

    def __init__(self, devices=None, misc=None, config=None, post_threads=2, keep_results=True):
        L = lib()
        self.misc = misc if misc is not None else default_misc()
        self.config = config if config is not None else default_config()
        self.results = {}
        self.order = []
        self.n_chains = 0
        self.n_kept = 0

        def on_done(_user, read_id, n_u, u, n_a, a):
            if not keep_results:                     # rate measurements: count, do not copy
                self.n_chains += n_u
                self.n_kept += n_a
                return
            uu = np.ctypeslib.as_array(u, shape=(n_u,)).copy() if n_u else np.zeros(0, np.uint64)
            aa = (np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_uint64)), shape=(n_a, 2)).copy() if n_a else np.zeros((0, 2), np.uint64))
            self.results[read_id] = (uu, aa)
            self.order.append(read_id)

        self._cb = READ_DONE_FN(on_done)          # keep alive
        ids = np.ascontiguousarray(devices, dtype=np.int32) if devices is not None else None
        self._h = L.mm2gb_batcher_create(C.byref(self.config), C.byref(self.misc), 0 if ids is None else len(ids),
                                         None if ids is None else ids.ctypes.data, post_threads, self._cb, None)
        if not self._h:
            raise Mm2gbError(L.mm2gb_last_error().decode())

    def add(self, read_id, anchors):
        a = np.ascontiguousarray(anchors, dtype=np.uint64)
        _check(lib().mm2gb_batcher_add(self._h, read_id, a.ctypes.data, len(a)))

    def feed(self, first_id, anchors, offsets, producers=1):
        """mm2gb_batcher_feed: the reads of a packed batch added one at a time by `producers` native threads (read r gets id first_id + r)."""
        a = np.ascontiguousarray(anchors, dtype=np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        L = lib()
        L.mm2gb_batcher_feed.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
        _check(L.mm2gb_batcher_feed(self._h, len(off) - 1, int(first_id), off.ctypes.data, a.ctypes.data, int(producers)))

    def flush(self):
        _check(lib().mm2gb_batcher_flush(self._h))

    def stats(self):
        st = BatcherStats()
        _check(lib().mm2gb_batcher_stats(self._h, C.byref(st)))
        return {"reads": st.reads, "anchors": st.anchors, "reads_per_lane": list(st.reads_per_lane), "batches": list(st.batches),
                "batches_per_engine": list(st.batches_per_engine)[: st.n_engines], "n_engines": st.n_engines}

    def close(self):
        if getattr(self, "_h", None):
            lib().mm2gb_batcher_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def backtrack_host(misc, anchors, f, p_rel):
    """mm2gb_backtrack_host: backtrack + compaction for one read from f / relative p."""
    a = np.ascontiguousarray(anchors, dtype=np.uint64)
    f = np.ascontiguousarray(f, dtype=np.int32)
    p = np.ascontiguousarray(p_rel, dtype=np.int32)
    u_ptr = C.c_void_p(0)
    a_ptr = C.c_void_p(0)
    L = lib()
    n_u = L.mm2gb_backtrack_host(C.byref(misc), len(f), a.ctypes.data, f.ctypes.data, p.ctypes.data, C.byref(u_ptr), C.byref(a_ptr))
    if n_u < 0:
        raise Mm2gbError(L.mm2gb_last_error().decode())
    if n_u == 0:
        return np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64)
    u = np.ctypeslib.as_array(C.cast(u_ptr, C.POINTER(C.c_uint64)), shape=(n_u,)).copy()
    n_out = int((u & 0xffffffff).sum())
    a_out = np.ctypeslib.as_array(C.cast(a_ptr, C.POINTER(C.c_uint64)), shape=(n_out, 2)).copy()
    L.mm2gb_free(u_ptr)
    L.mm2gb_free(a_ptr)
    return u, a_out


def synth_count(seed, first_read, n_reads, len_lo, len_hi):
    """How many anchors synth_reads would make for these reads (no anchors are generated)."""
    L = lib()
    off = np.zeros(n_reads + 1, dtype=np.int64)
    n = L.mm2gb_synth_count(seed, first_read, n_reads, len_lo, len_hi, off.ctypes.data)
    if n < 0:
        raise Mm2gbError(L.mm2gb_last_error().decode())
    return int(n)


def synth_reads(seed, first_read, n_reads, len_lo, len_hi, threads=8):
    """Deterministic synthetic reads.  Returns anchors (n,2) uint64 and offsets (R+1,) int64."""
    L = lib()
    off = np.zeros(n_reads + 1, dtype=np.int64)
    n = L.mm2gb_synth_count(seed, first_read, n_reads, len_lo, len_hi, off.ctypes.data)
    if n < 0:
        raise Mm2gbError(L.mm2gb_last_error().decode())
    a = np.empty((n, 2), dtype=np.uint64)
    _check(L.mm2gb_synth_fill(seed, first_read, n_reads, len_lo, len_hi, off.ctypes.data, a.ctypes.data, threads))
    return a, off


# ---- from sequence to seed matches on the host (csrc/seeding.cpp) ------------------------------------------------------------
class SeedOpt(C.Structure):
    _fields_ = [("mid_occ", C.c_int32), ("max_max_occ", C.c_int32), ("occ_dist", C.c_int32), ("q_occ_frac", C.c_float)]


class Matches(C.Structure):
    _fields_ = [("n_seeds", C.c_int32), ("rep_len", C.c_int32), ("n_mini_pos", C.c_int32), ("pad_", C.c_int32), ("n_hits", C.c_int64),
                ("seeds", C.c_void_p), ("hits", C.c_void_p), ("mini_pos", C.c_void_p)]


I_HPC = 0x1    # MM2GB_I_HPC


def preset(name):
    """The index and seeding parameters of a minimap2 preset, as keywords for SeedIndex (k, w, hpc) and map_reads (k).  "map-pb" (alias
    "map10k"): -H -k19 (options.c:102-103), w = 10.  "splice" / "cdna" / "splice:hq": -k15 -w5 (options.c:152); their alignment options are
    align_splice_opt's.  "map-hifi" / "map-ccs", "asm5", "asm10": -k19 -w19; "asm20": -k19 -w10 (options.c:110-131); their mapping options are
    map_opt_preset's, their alignment options align_opt's.  No other preset: their mapping options are not the mapper's."""
    if name in ("map-pb", "map10k"):
        return dict(k=19, w=10, hpc=True)
    if name in ("map-hifi", "map-ccs", "asm5", "asm10"):
        return dict(k=19, w=19, hpc=False)
    if name == "asm20":
        return dict(k=19, w=10, hpc=False)
    if name in ("splice", "cdna", "splice:hq"):
        return dict(k=15, w=5, hpc=False)
    raise Mm2gbError(f"preset {name!r} is not supported (map-pb / map10k, splice / cdna / splice:hq, map-hifi / map-ccs, asm5, asm10, asm20)")


def sketch(seq, w=10, k=15, rid=0, hpc=False):
    """mm2gb_sketch: the (w,k)-minimizers of a sequence (bytes) as an (n,2) uint64 array (x = hash << 8 | span, y = rid << 32 | pos << 1 | strand).
    hpc: homopolymer-compressed (mm2gb_sketch_flag with MM2GB_I_HPC): pos is the last base of the k-mer's last run, span the bases it covers."""
    ptr, n = C.c_void_p(), C.c_int64()
    if hpc:
        _check(lib().mm2gb_sketch_flag(seq, len(seq), w, k, rid, I_HPC, C.byref(ptr), C.byref(n)))
    else:
        _check(lib().mm2gb_sketch(seq, len(seq), w, k, rid, C.byref(ptr), C.byref(n)))
    out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(max(n.value, 1) * 2,))[:n.value * 2].reshape(-1, 2).copy()
    lib().mm2gb_free(ptr)
    return out


class IndexView(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("n_occ", C.c_int64), ("n_bucket", C.c_int64), ("bucket_shift", C.c_int32), ("k", C.c_int32), ("w", C.c_int32),
                ("built_on", C.c_int32), ("uploads", C.c_int64), ("keys", C.c_void_p), ("first", C.c_void_p), ("where", C.c_void_p), ("bucket", C.c_void_p)]


class SeedIndex:
    """Minimizer index of reference sequences (list of bytes) with the look-up semantics of the reference's mm_idx_get.  With an engine the
    index is built on that engine's device (mm2gb_index_build_gpu) and stays resident there; its arrays are the host build's.  hpc: the
    minimizers are homopolymer-compressed; the index owns that choice: reads matched or mapped against it are sketched the same way."""

    def __init__(self, seqs, k=15, w=10, threads=4, engine=None, hpc=False):
        self._seqs = [bytes(s) for s in seqs]
        arr = (C.c_char_p * len(self._seqs))(*self._seqs)
        lens = np.ascontiguousarray([len(s) for s in self._seqs], dtype=np.int32)
        self.lens = lens
        if hpc:
            if engine is not None:
                self._h = lib().mm2gb_index_build_gpu_flag(engine._h, k, w, I_HPC, len(self._seqs), arr, lens.ctypes.data)
            else:
                self._h = lib().mm2gb_index_build_flag(k, w, I_HPC, len(self._seqs), arr, lens.ctypes.data, threads)
        elif engine is not None:
            self._h = lib().mm2gb_index_build_gpu(engine._h, k, w, len(self._seqs), arr, lens.ctypes.data)
        else:
            self._h = lib().mm2gb_index_build(k, w, len(self._seqs), arr, lens.ctypes.data, threads)
        if not self._h:
            raise Mm2gbError(lib().mm2gb_last_error().decode())

    @property
    def hpc(self):
        """Whether the index holds homopolymer-compressed minimizers (mm2gb_index_flag & MM2GB_I_HPC)."""
        flag = int(lib().mm2gb_index_flag(self._h))
        if flag < 0:
            raise Mm2gbError(lib().mm2gb_last_error().decode())
        return bool(flag & I_HPC)

    def close(self):
        if self._h:
            lib().mm2gb_index_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def size(self):
        occ = C.c_int64()
        return int(lib().mm2gb_index_size(self._h, C.byref(occ))), int(occ.value)

    def mid_occ(self, frac=2e-4, min_mid_occ=10, max_mid_occ=1000000, engine=None):
        """mm2gb_index_mid_occ; with an engine mm2gb_index_mid_occ_gpu: the same value, the quantile found on the engine's device."""
        if engine is None:
            return int(lib().mm2gb_index_mid_occ(self._h, frac, min_mid_occ, max_mid_occ))
        occ = int(lib().mm2gb_index_mid_occ_gpu(engine._h, self._h, frac, min_mid_occ, max_mid_occ))
        if occ < 0:
            raise Mm2gbError(lib().mm2gb_last_error().decode())
        return occ

    def _raw_view(self):
        v = IndexView()
        _check(lib().mm2gb_index_view(self._h, C.byref(v)))
        return v

    def view(self):
        """mm2gb_index_view: dict of numpy copies of keys / first / where / bucket and the scalars n_keys, n_occ, n_bucket, bucket_shift, k, w,
        built_on (the device the index was built on, or -1) and uploads (host -> device copies made for it so far)."""
        v = self._raw_view()
        out = {f: int(getattr(v, f)) for f in ("n_keys", "n_occ", "n_bucket", "bucket_shift", "k", "w", "built_on", "uploads")}
        out.update(keys=_take(v.keys, v.n_keys, np.uint64), first=_take(v.first, v.n_keys + 1, np.int64), where=_take(v.where, v.n_occ, np.uint64),
                   bucket=_take(v.bucket, v.n_bucket, np.uint32))
        return out

    def fetch_device(self, device):
        """mm2gb_index_fetch_device: the arrays resident on a device, as dict(keys, first, where, bucket); an error if none are."""
        v = self._raw_view()
        out = dict(keys=np.zeros(v.n_keys, np.uint64), first=np.zeros(v.n_keys + 1, np.int64), where=np.zeros(v.n_occ, np.uint64),
                   bucket=np.zeros(v.n_bucket, np.uint32))
        _check(lib().mm2gb_index_fetch_device(self._h, int(device), out["keys"].ctypes.data, out["first"].ctypes.data, out["where"].ctypes.data,
                                              out["bucket"].ctypes.data))
        return out

    def build_split(self):
        """mm2gb_index_build_split: milliseconds of the device build's stages (zeros for a host build)."""
        ms = (C.c_double * 5)()
        _check(lib().mm2gb_index_build_split(self._h, ms))
        return dict(zip(("h2d", "sketch", "sort", "tables", "d2h"), (float(x) for x in ms)))

    def matches(self, seq, mid_occ, max_max_occ=4095, occ_dist=500, q_occ_frac=0.01):
        """mm2gb_collect_matches for one read: dict(seeds (n,4) uint32, hits uint64, qlen, rep_len, mini_pos) -- the record Engine.collect_seeds takes."""
        opt = SeedOpt(int(mid_occ), int(max_max_occ), int(occ_dist), float(q_occ_frac))
        m = Matches()
        _check(lib().mm2gb_collect_matches(self._h, bytes(seq), len(seq), C.byref(opt), C.byref(m)))
        def take(ptr, n, dt):
            if n == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dt).itemsize,)).view(dt).copy()
        out = dict(seeds=take(m.seeds, m.n_seeds * 4, np.uint32).reshape(-1, 4), hits=take(m.hits, m.n_hits, np.uint64), qlen=len(seq),
                   rep_len=int(m.rep_len), mini_pos=take(m.mini_pos, m.n_mini_pos, np.uint64))
        lib().mm2gb_matches_free(C.byref(m))
        return out

    def matches_frag(self, mates, mid_occ, max_max_occ=4095, occ_dist=500, q_occ_frac=0.01):
        """mm2gb_collect_matches_frag for one fragment: mates = one or two sequences (bytes; a mate that pe_ori turns is given turned), seeded as one list of their summed
        length (the second mate's seeds carry segment id 1 in seeds[:, 3] and positions past the first mate).  The dict matches() returns, qlen the summed length."""
        mates = [bytes(s) for s in mates]
        opt = SeedOpt(int(mid_occ), int(max_max_occ), int(occ_dist), float(q_occ_frac))
        m = Matches()
        arr = (C.c_char_p * max(len(mates), 1))(*mates)
        lens = np.ascontiguousarray([len(s) for s in mates], dtype=np.int32)
        fn = lib().mm2gb_collect_matches_frag
        fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(SeedOpt), C.POINTER(Matches)]
        _check(fn(self._h, len(mates), arr, lens.ctypes.data, C.byref(opt), C.byref(m)))
        out = dict(seeds=_take(m.seeds, m.n_seeds * 4, np.uint32).reshape(-1, 4), hits=_take(m.hits, m.n_hits, np.uint64), qlen=int(lens.sum()),
                   rep_len=int(m.rep_len), mini_pos=_take(m.mini_pos, m.n_mini_pos, np.uint64))
        lib().mm2gb_matches_free(C.byref(m))
        return out


class MatchBatch(C.Structure):
    _fields_ = [("n_seeds", C.c_int64), ("n_hits", C.c_int64), ("seed_off", C.c_void_p), ("seeds", C.c_void_p), ("hit_off", C.c_void_p),
                ("hits", C.c_void_p), ("mini_pos", C.c_void_p), ("rep_len", C.c_void_p)]


def _lay_end_to_end(seqs):
    seqs = [bytes(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return seqs, off, b"".join(seqs)


def _take(ptr, n, dt):
    if n == 0:
        return np.zeros(0, dt)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dt).itemsize,)).view(dt).copy()


def _engine_sketch(self, seqs, w=10, k=15, rid=None, hpc=False):
    """mm2gb_sketch_gpu: the (w,k)-minimizers of a list of sequences (bytes) on the device: one (n,2) uint64 array per sequence, equal to
    sketch(seq, w, k, rid[r], hpc)."""
    seqs, off, flat = _lay_end_to_end(seqs)
    rids = np.ascontiguousarray(rid, dtype=np.uint32) if rid is not None else None
    mini_off = np.zeros(len(seqs) + 1, np.int64)
    ptr = C.c_void_p()
    if hpc:
        _check(lib().mm2gb_sketch_gpu_flag(self._h, int(w), int(k), I_HPC, len(seqs), off.ctypes.data, flat, rids.ctypes.data if rids is not None else None,
                                           mini_off.ctypes.data, C.byref(ptr)))
    else:
        _check(lib().mm2gb_sketch_gpu(self._h, int(w), int(k), len(seqs), off.ctypes.data, flat, rids.ctypes.data if rids is not None else None,
                                      mini_off.ctypes.data, C.byref(ptr)))
    xy = _take(ptr, int(mini_off[-1]) * 2, np.uint64).reshape(-1, 2)
    lib().mm2gb_free(ptr)
    return [xy[mini_off[r]:mini_off[r + 1]] for r in range(len(seqs))]


def _engine_collect_matches(self, index, seqs, mid_occ, max_max_occ=4095, occ_dist=500, q_occ_frac=0.01):
    """mm2gb_collect_matches_gpu: for every read (bytes) the dict SeedIndex.matches returns, computed on the device in one call."""
    seqs, off, flat = _lay_end_to_end(seqs)
    opt = SeedOpt(int(mid_occ), int(max_max_occ), int(occ_dist), float(q_occ_frac))
    m = MatchBatch()
    _check(lib().mm2gb_collect_matches_gpu(self._h, index._h if index is not None else None, C.byref(opt), len(seqs), off.ctypes.data, flat, C.byref(m)))
    R = len(seqs)
    seed_off = _take(m.seed_off, R + 1, np.int64)
    seeds = _take(m.seeds, m.n_seeds * 4, np.uint32).reshape(-1, 4)
    hit_off = _take(m.hit_off, m.n_seeds + 1, np.int64)
    hits = _take(m.hits, m.n_hits, np.uint64)
    mini_pos = _take(m.mini_pos, m.n_seeds, np.uint64)
    rep_len = _take(m.rep_len, R, np.int32)
    lib().mm2gb_match_batch_free(C.byref(m))
    return [dict(seeds=seeds[seed_off[r]:seed_off[r + 1]], hits=hits[hit_off[seed_off[r]]:hit_off[seed_off[r + 1]]], qlen=len(seqs[r]),
                 rep_len=int(rep_len[r]), mini_pos=mini_pos[seed_off[r]:seed_off[r + 1]]) for r in range(R)]


def _engine_collect_matches_frag(self, index, frags, mid_occ, max_max_occ=4095, occ_dist=500, q_occ_frac=0.01):
    """mm2gb_collect_matches_frag_gpu: frags = a list of fragments, each a list of one or two sequences (bytes); for every fragment the dict SeedIndex.matches_frag
    returns, computed on the device in one call."""
    frags = [[bytes(s) for s in f] for f in frags]
    seqs, off, flat = _lay_end_to_end([s for f in frags for s in f])
    frag_off = np.zeros(len(frags) + 1, np.int64)
    frag_off[1:] = np.cumsum([len(f) for f in frags])
    opt = SeedOpt(int(mid_occ), int(max_max_occ), int(occ_dist), float(q_occ_frac))
    m = MatchBatch()
    fn = lib().mm2gb_collect_matches_frag_gpu
    fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SeedOpt), C.c_int64, C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.POINTER(MatchBatch)]
    _check(fn(self._h, index._h if index is not None else None, C.byref(opt), len(seqs), off.ctypes.data, flat, len(frags), frag_off.ctypes.data, C.byref(m)))
    R = len(frags)
    seed_off = _take(m.seed_off, R + 1, np.int64)
    seeds = _take(m.seeds, m.n_seeds * 4, np.uint32).reshape(-1, 4)
    hit_off = _take(m.hit_off, m.n_seeds + 1, np.int64)
    hits = _take(m.hits, m.n_hits, np.uint64)
    mini_pos = _take(m.mini_pos, m.n_seeds, np.uint64)
    rep_len = _take(m.rep_len, R, np.int32)
    lib().mm2gb_match_batch_free(C.byref(m))
    return [dict(seeds=seeds[seed_off[r]:seed_off[r + 1]], hits=hits[hit_off[seed_off[r]]:hit_off[seed_off[r + 1]]], qlen=sum(len(s) for s in frags[r]),
                 rep_len=int(rep_len[r]), mini_pos=mini_pos[seed_off[r]:seed_off[r + 1]]) for r in range(R)]


Engine.sketch = _engine_sketch
Engine.collect_matches = _engine_collect_matches
Engine.collect_matches_frag = _engine_collect_matches_frag


class MapOpt(C.Structure):
    _fields_ = [("flag", C.c_int64), ("seed", C.c_int32), ("mid_occ", C.c_int32), ("min_mid_occ", C.c_int32), ("max_mid_occ", C.c_int32),
                ("max_max_occ", C.c_int32), ("occ_dist", C.c_int32), ("mid_occ_frac", C.c_float), ("q_occ_frac", C.c_float),
                ("min_cnt", C.c_int32), ("min_chain_score", C.c_int32), ("bw", C.c_int32), ("bw_long", C.c_int32), ("max_gap", C.c_int32),
                ("max_gap_ref", C.c_int32), ("max_chain_iter", C.c_int32), ("rmq_inner_dist", C.c_int32), ("rmq_size_cap", C.c_int32),
                ("rmq_rescue_size", C.c_int32), ("rmq_rescue_ratio", C.c_float), ("chain_gap_scale", C.c_float), ("chain_skip_scale", C.c_float),
                ("mask_level", C.c_float), ("mask_len", C.c_int32), ("pri_ratio", C.c_float), ("best_n", C.c_int32), ("host_threads", C.c_int32), ("seeds_on_device", C.c_int32), ("rechain_on_device", C.c_int32),
                ("max_chain_skip", C.c_int32), ("seeding_on_device", C.c_int32)]


class MapStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_reads", "n_mapped", "n_anchors", "n_chains", "n_rechained", "n_rmq_tied")] + \
               [(k, C.c_double) for k in ("s_seed", "s_anchors", "s_chain", "s_rechain", "s_regs", "s_post")]

    def as_dict(self):
        return {k: (round(getattr(self, k), 4) if k.startswith("s_") else int(getattr(self, k))) for k, _ in self._fields_}


def map_opt(**kw):
    o = MapOpt()
    lib().mm2gb_map_opt_init(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


F_RMQ = 0x80000000      # MM2GB_F_RMQ (MM_F_RMQ): mg_lchain_rmq as the first chainer; what the asm presets set


def map_opt_preset(name, **kw):
    """mm2gb_map_opt_init_preset: the mapping fields of "map-ont", "map-pb", "map-hifi" / "map-ccs", "asm5", "asm10" or "asm20" (the asm presets set
    F_RMQ, bw = 1000, bw_long = 100000, best_n = 50), then keyword overrides.  Use an index built with **preset(name) and align=map_align(refs, preset=name)."""
    o = MapOpt()
    fn = lib().mm2gb_map_opt_init_preset
    fn.argtypes = [C.POINTER(MapOpt), C.c_char_p]
    _check(fn(C.byref(o), name.encode()))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise Mm2gbError(f"mm2gb_map_opt_t has no field {k!r}")
        setattr(o, k, v)
    return o


# read against read (minimap2 -X = the four together; main.c:176-178): MM2GB_F_NO_DIAG, _NO_DUAL, _NO_LJOIN, _ALL_CHAINS
F_NO_DIAG, F_NO_DUAL, F_NO_LJOIN, F_ALL_CHAINS = 0x001, 0x002, 0x400, 0x800000
SEEDING_RESIDENT = 2    # MM2GB_SEEDING_RESIDENT: seeding_on_device's value for the resident path (anchors and chains never leave the device)


def map_opt_ava(name, **kw):
    """mm2gb_map_opt_init_ava: the mapping fields of "ava-ont" or "ava-pb" (options.c:96-109: the four read-overlap bits, min_chain_score = 100, pri_ratio = 0,
    occ_dist = 0; ava-ont bw = bw_long = 2000, ava-pb bw_long = bw), then keyword overrides.  Use an index built with **preset_ava(name), and no align=."""
    o = MapOpt()
    fn = lib().mm2gb_map_opt_init_ava
    fn.argtypes = [C.POINTER(MapOpt), C.c_char_p]
    _check(fn(C.byref(o), name.encode()))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise Mm2gbError(f"mm2gb_map_opt_t has no field {k!r}")
        setattr(o, k, v)
    return o


def preset_ava(name):
    """The index parameters of the read-overlap presets, as keywords for SeedIndex and map_reads: "ava-ont" -k15 -w5, "ava-pb" -Hk19 -w5 (options.c:96-109)."""
    if name == "ava-ont":
        return dict(k=15, w=5, hpc=False)
    if name == "ava-pb":
        return dict(k=19, w=5, hpc=True)
    raise Mm2gbError(f"preset_ava: {name!r} is not supported (ava-ont, ava-pb)")


# short single-end reads (minimap2 -x sr): MM2GB_F_SR, _FRAG_MODE, _NO_PRINT_2ND, _HEAP_SORT
F_SR, F_FRAG_MODE, F_NO_PRINT_2ND, F_HEAP_SORT = 0x1000, 0x2000, 0x4000, 0x400000


def map_opt_sr(**kw):
    """mm2gb_map_opt_init_sr: the mapping fields of "sr" / "short" (options.c:133-150: the four bits above, max_gap = bw = bw_long = 100, pri_ratio = 0.5, min_cnt = 2,
    min_chain_score = 25, best_n = 20, mid_occ = 1000), then keyword overrides.  For map_reads(..., opt=map_opt_sr(), k=21, align=map_sr()); without align=map_sr()
    map_reads refuses these flags as before.  The index: **preset_sr()."""
    o = MapOpt()
    fn = lib().mm2gb_map_opt_init_sr
    fn.argtypes = [C.POINTER(MapOpt)]
    fn.restype = None
    fn(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise Mm2gbError(f"mm2gb_map_opt_t has no field {k!r}")
        setattr(o, k, v)
    return o


def preset_sr():
    """The index parameters of the short-read preset, as keywords for SeedIndex: -k21 -w11, no HPC (options.c:134)."""
    return dict(k=21, w=11, hpc=False)


class EstErr(C.Structure):
    _fields_ = [("n_match", C.c_int32), ("n_tot", C.c_int32)]


def _est_err_call(fn, head, reads, ref_len, tail):
    """The arguments of mm2gb_est_err_host / _gpu from reads: a list of dicts with hits (list of dicts: as, cnt, rid, qs, rs, re, rev), anchors ((n,2) uint64), qlen,
    mini_pos (uint64).  Returns the offsets, the result arrays, the call's arguments before and after the form's own, and the arrays to keep alive."""
    R = len(reads)
    reg_off, a_off, m_off = (np.zeros(R + 1, dtype=np.int64) for _ in range(3))
    for r, rd in enumerate(reads):
        reg_off[r + 1] = reg_off[r] + len(rd["hits"])
        a_off[r + 1] = a_off[r] + len(rd["anchors"])
        m_off[r + 1] = m_off[r] + len(rd["mini_pos"])
    regs = np.zeros(max(int(reg_off[R]), 1), dtype=REG_DTYPE)
    j = 0
    for rd in reads:
        for h in rd["hits"]:
            for k in ("cnt", "rid", "qs", "rs", "re"):
                regs[j][k] = h[k]
            regs[j]["as_"] = h["as"]
            regs[j]["flags"] = (1 << 10) if h.get("rev") else 0
            j += 1
    anchors = np.ascontiguousarray(np.concatenate([np.asarray(rd["anchors"], dtype=np.uint64).reshape(-1, 2) for rd in reads] + [np.zeros((1, 2), dtype=np.uint64)]))
    mini = np.ascontiguousarray(np.concatenate([np.asarray(rd["mini_pos"], dtype=np.uint64).reshape(-1) for rd in reads] + [np.zeros(1, dtype=np.uint64)]))
    qlen = np.ascontiguousarray([rd["qlen"] for rd in reads] + [0], dtype=np.int32)
    rl = np.ascontiguousarray(ref_len, dtype=np.int32)
    out = np.zeros((max(int(reg_off[R]), 1), 2), dtype=np.int32)
    sum_k = np.zeros(R + 1, dtype=np.uint64)
    fn.argtypes = head + [C.c_int64] + [C.c_void_p] * 7 + [C.c_int32, C.c_void_p] + tail + [C.c_void_p, C.c_void_p]
    return reg_off, m_off, out, sum_k, (R, reg_off.ctypes.data, regs.ctypes.data, a_off.ctypes.data, anchors.ctypes.data, qlen.ctypes.data, m_off.ctypes.data, mini.ctypes.data,
                                        len(rl), rl.ctypes.data), (out.ctypes.data, sum_k.ctypes.data), (regs, anchors, mini, qlen, rl, a_off)


def _est_err_result(reg_off, m_off, out, sum_k):
    """Per read a dict with n_match, n_tot (int32 arrays, one entry per hit; n_tot = -1: the walk did not start), sum_k and div (float32: mm2gb_est_err_div on them)."""
    L = lib()
    L.mm2gb_est_err_div.argtypes = [C.c_int32, C.c_int32, C.c_uint64, C.c_int32]
    L.mm2gb_est_err_div.restype = C.c_float
    res = []
    for r in range(len(reg_off) - 1):
        o = out[reg_off[r]:reg_off[r + 1]]
        n_mini = int(m_off[r + 1] - m_off[r])
        div = np.asarray([L.mm2gb_est_err_div(int(a), int(b), int(sum_k[r]), n_mini) for a, b in o], dtype=np.float32)
        res.append(dict(n_match=o[:, 0].copy(), n_tot=o[:, 1].copy(), sum_k=int(sum_k[r]), div=div))
    return res


def est_err_host(reads, ref_len, threads=4):
    """mm2gb_est_err_host: mm_est_err's walk (esterr.c:30-61) on host threads; reads as _est_err_call takes them, ref_len per reference sequence; result as
    _est_err_result gives it."""
    fn = lib().mm2gb_est_err_host
    reg_off, m_off, out, sum_k, first, last, keep = _est_err_call(fn, [], reads, ref_len, [C.c_int])
    _check(fn(*first, int(threads), *last))
    return _est_err_result(reg_off, m_off, out, sum_k)


def _engine_est_err(self, reads, ref_len):
    """mm2gb_est_err_gpu: the same on the device (k_est_err)."""
    fn = lib().mm2gb_est_err_gpu
    reg_off, m_off, out, sum_k, first, last, keep = _est_err_call(fn, [C.c_void_p], reads, ref_len, [])
    _check(fn(self._h, *first, *last))
    return _est_err_result(reg_off, m_off, out, sum_k)


Engine.est_err = _engine_est_err


class MapAln(C.Structure):
    """mm2gb_map_aln_t: what mm2gb_map_reads_aln needs beside the mapping options (make one with map_align)."""
    _fields_ = [("ref_seqs", C.POINTER(C.c_char_p)), ("opt", AlignOpt), ("what", C.c_int32), ("align_on_device", C.c_int32), ("text_on_device", C.c_int32)]


def map_align(refs, preset="map-ont", cigar=True, cs=None, md=False, align_on_device=0, text_on_device=0, **align_opt_fields):
    """Base-level alignment for map_reads / map_reads_stream (their align= argument; minimap2 -c): refs: the reference sequences as bytes, in the
    index's order; preset: any name align_opt takes, keyword overrides for its fields; cigar: cg:Z; cs: None, "short" or "long"
    (--cs, --cs=long); md: MD:Z (--MD; it is written instead of cs when both are asked for, as by minimap2).  align_on_device / text_on_device:
    1 the device form, -1 host threads, 0 the default (alignment on the device; text on host threads)."""
    if cs not in (None, "short", "long"):
        raise Mm2gbError('map_align: cs is None, "short" or "long"')
    a = MapAln()
    a._refs = [bytes(s) for s in refs]                                                  # (kept alive with the structure)
    a._arr = (C.c_char_p * max(len(a._refs), 1))(*a._refs)
    a.ref_seqs = C.cast(a._arr, C.POINTER(C.c_char_p))
    a.opt = align_opt(preset, **align_opt_fields)
    a.what = (TEXT_CG if cigar else 0) | (TEXT_CS if cs else 0) | (TEXT_CS_LONG if cs == "long" else 0) | (TEXT_MD if md else 0)
    a.align_on_device, a.text_on_device = int(align_on_device), int(text_on_device)
    return a


class MapSplice(C.Structure):
    """mm2gb_map_splice_t: what mm2gb_map_reads_splice needs beside the mapping options (make one with map_splice)."""
    _fields_ = [("ref_seqs", C.POINTER(C.c_char_p)), ("opt", AlignSpliceOpt), ("what", C.c_int32), ("align_on_device", C.c_int32), ("text_on_device", C.c_int32)]


def map_splice(refs, preset="splice", cigar=True, cs=None, md=False, align_on_device=0, text_on_device=0, **align_opt_fields):
    """Spliced base-level alignment for map_reads / map_reads_stream (their align= argument; minimap2 -x splice -c): map_align's arguments with
    preset "splice", "cdna" or "splice:hq" (align_splice_opt).  Use opt=map_opt_splice() and an index built with **preset("splice")."""
    if cs not in (None, "short", "long"):
        raise Mm2gbError('map_splice: cs is None, "short" or "long"')
    a = MapSplice()
    a._refs = [bytes(s) for s in refs]
    a._arr = (C.c_char_p * max(len(a._refs), 1))(*a._refs)
    a.ref_seqs = C.cast(a._arr, C.POINTER(C.c_char_p))
    a.opt = align_splice_opt(preset, **align_opt_fields)
    a.what = (TEXT_CG if cigar else 0) | (TEXT_CS if cs else 0) | (TEXT_CS_LONG if cs == "long" else 0) | (TEXT_MD if md else 0)
    a.align_on_device, a.text_on_device = int(align_on_device), int(text_on_device)
    return a


def map_opt_splice(**kw):
    """mm2gb_map_opt_init_splice (the `splice` presets' mapping fields: bw = bw_long = max_gap_ref = 200000, max_gap = 2000), then keyword overrides."""
    o = MapOpt()
    lib().mm2gb_map_opt_init_splice(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _check_align_refs(align, ref_names):
    if len(align._refs) != len(ref_names):
        raise Mm2gbError("map_reads: align holds another number of reference sequences than ref_names")


def _stats_with_extra(st, extra):
    return dict(st.as_dict(), s_align=round(extra[0], 4), s_post_align=round(extra[1], 4), s_text=round(extra[2], 4))


class MapSr(C.Structure):
    """mm2gb_map_sr_t: what mm2gb_map_reads_sr needs beside the mapping options (make one with map_sr)."""
    _fields_ = [("ref_seqs", C.POINTER(C.c_char_p)), ("opt", AlignOpt), ("align", C.c_int32), ("what", C.c_int32), ("align_on_device", C.c_int32), ("text_on_device", C.c_int32),
                ("max_occ", C.c_int32), ("max_frag_len", C.c_int32)]


class MapSrOut(C.Structure):
    """mm2gb_map_sr_out_t: the short-read calls' own counts and seconds."""
    _fields_ = [("n_chain_calls", C.c_int64), ("n_rescued", C.c_int64), ("n_tied_reads", C.c_int64), ("sr_counts", C.c_int64 * len(SR_COUNTS)), ("s_extra", C.c_double * 3)]


def map_sr(refs=None, align=False, cs=None, md=False, align_on_device=0, text_on_device=0, **fields):
    """Short single-end reads for map_reads / map_reads_stream (their align= argument; minimap2 -x sr): mm2gb_map_sr_init's values (max_occ = 5000, max_frag_len = 800,
    align_sr_opt()'s alignment values), then keyword overrides of max_occ / max_frag_len or of a field of the alignment's option set.  align=True: base-level alignment
    (minimap2 -c; refs: the reference sequences as bytes, in the index's order) with cg:Z; cs: None, "short" or "long"; md: MD:Z.  align_on_device / text_on_device as
    for map_align.  Use opt=map_opt_sr(), k=21 and an index built with **preset_sr()."""
    if cs not in (None, "short", "long"):
        raise Mm2gbError('map_sr: cs is None, "short" or "long"')
    if align and refs is None:
        raise Mm2gbError("map_sr: align=True needs refs, the reference sequences")
    a = MapSr()
    fn = lib().mm2gb_map_sr_init
    fn.argtypes = [C.POINTER(MapSr)]
    fn.restype = None
    fn(C.byref(a))
    if refs is not None:
        a._refs = [bytes(s) for s in refs]
        a._arr = (C.c_char_p * max(len(a._refs), 1))(*a._refs)
        a.ref_seqs = a._arr
    a.align = 1 if align else 0
    a.what = (TEXT_CG if align else 0) | ({None: 0, "short": TEXT_CS, "long": TEXT_CS | TEXT_CS_LONG}[cs]) | (TEXT_MD if md else 0)
    a.align_on_device, a.text_on_device = int(align_on_device), int(text_on_device)
    for k, v in fields.items():
        if k in ("max_occ", "max_frag_len"):
            setattr(a, k, v)
        elif hasattr(a.opt, k):
            setattr(a.opt, k, v)
        else:
            raise Mm2gbError(f"map_sr: no field {k!r} (max_occ, max_frag_len, or a field of mm2gb_align_opt_t)")
    return a


def _sr_stats(st, so):
    return dict(st.as_dict(), n_chain_calls=int(so.n_chain_calls), n_rescued=int(so.n_rescued), n_tied_reads=int(so.n_tied_reads),
                sr_counts=dict(zip(SR_COUNTS, (int(x) for x in so.sr_counts))), s_align=round(so.s_extra[0], 4), s_post_align=round(so.s_extra[1], 4), s_text=round(so.s_extra[2], 4))


class MapOut(C.Structure):
    """mm2gb_map_out_t: SAM output and = / X CIGARs from the mapping calls that align (make one with map_out)."""
    _fields_ = [("format", C.c_int32), ("eqx_on_device", C.c_int32), ("flag", C.c_int64)]


F_SOFTCLIP, F_SAM_HIT_ONLY = 0x80000, 0x40000000


def map_out(sam=False, eqx=False, softclip=False, hit_only=False, eqx_on_device=0):
    """The out= argument of map_reads / map_reads_stream (with an align= that aligns): sam: SAM lines (minimap2 -a; sam_header gives the header);
    eqx: = / X in the CIGAR column or cg:Z (--eqx); softclip: S clips and the whole SEQ on supplementary lines (-Y); hit_only: no line for a read
    without a hit (--sam-hit-only).  eqx_on_device: 1 the device form of the rewrite, -1 host threads, 0 the default (host threads)."""
    o = MapOut()
    lib().mm2gb_map_out_init.argtypes = [C.POINTER(MapOut)]
    lib().mm2gb_map_out_init.restype = None
    lib().mm2gb_map_out_init(C.byref(o))
    o.format = 1 if sam else 0
    o.flag = (F_EQX if eqx else 0) | (F_SOFTCLIP if softclip else 0) | (F_SAM_HIT_ONLY if hit_only else 0)
    o.eqx_on_device = int(eqx_on_device)
    return o


def sam_header(ref_names, ref_lens):
    """mm2gb_sam_header: the @SQ line of every reference and this project's @PG line, as text."""
    L = lib()
    L.mm2gb_sam_header.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    rn = (C.c_char_p * max(len(ref_names), 1))(*[n.encode() for n in ref_names])
    lens = np.ascontiguousarray(ref_lens, dtype=np.int32)
    if len(lens) != len(ref_names):
        raise Mm2gbError("sam_header: one length per name")
    out, n = C.c_void_p(), C.c_int64()
    _check(L.mm2gb_sam_header(len(ref_names), rn, lens.ctypes.data, C.byref(out), C.byref(n)))
    text = C.string_at(out, n.value).decode()
    L.mm2gb_free(out)
    return text


def _out_needs_align(out, align):
    if out is not None and align is None and (out.format or out.flag & F_EQX):
        raise Mm2gbError("map_reads: SAM output and eqx need base-level alignment, an align= argument (minimap2 -a implies -c)")


def frag_offsets(names):
    """mm2gb_frag_offsets: where the fragments of a list of read names begin (one more entry than fragments, the last one len(names)): a run of consecutive reads with
    the same name is a fragment, a trailing "/" + digit not being part of the name (the reference's mm_qname_same)."""
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() if isinstance(n, str) else bytes(n) for n in names])
    off = np.zeros(len(names) + 1, np.int32)
    n = C.c_int32()
    fn = lib().mm2gb_frag_offsets
    fn.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(C.c_int32)]
    _check(fn(len(names), arr, off.ctypes.data, C.byref(n)))
    return off[:n.value + 1].copy()


def interleave(reads1, reads2):
    """Two files of mates as the one list the mapping calls take: reads1[0], reads2[0], reads1[1], ...; both lists of (name, sequence), equally long."""
    if len(reads1) != len(reads2):
        raise Mm2gbError("interleave: the two lists differ in length")
    return [r for pair in zip(reads1, reads2) for r in pair]


class SegOut(C.Structure):
    _fields_ = [("reg_off", C.c_void_p), ("regs", C.c_void_p), ("anchor_off", C.c_void_p), ("anchors", C.c_void_p)]


def _frag_arrays(n_segs, qlens):
    ns = np.ascontiguousarray(n_segs, dtype=np.int32)
    ql = np.zeros((len(ns), 2), np.int32)
    for f, q in enumerate(qlens):
        ql[f, :min(len(q), 2)] = q[:2]                     # (a fragment of three: n_segs says so, and the call refuses it)
    return ns, ql


def select_sub_multi_host(regs, qlens, max_gap_ref, pri_ratio=0.5, pri1=0.2, pri2=0.7, min_diff=42, best_n=20):
    """mm2gb_select_sub_multi_host (mm_select_sub_multi, pe.c:6-43): regs = per fragment a REG_DTYPE array after mm_set_parent, qlens = per fragment its one or two
    mate lengths, max_gap_ref = per fragment the chaining call's max_dist_x.  Returns per fragment the records that stay, ids and parents re-synchronised."""
    ns, ql = _frag_arrays([len(q) for q in qlens], qlens)
    off = np.concatenate([[0], np.cumsum([len(r) for r in regs])]).astype(np.int64)
    flat = np.concatenate([np.asarray(r, REG_DTYPE) for r in regs]) if len(regs) and off[-1] else np.zeros(0, REG_DTYPE)
    flat = np.ascontiguousarray(flat)
    gap = np.ascontiguousarray(max_gap_ref, dtype=np.int32)
    kept = np.zeros(max(len(ns), 1), np.int32)
    fn = lib().mm2gb_select_sub_multi_host
    fn.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(fn(pri_ratio, pri1, pri2, int(min_diff), int(best_n), len(ns), ns.ctypes.data, ql.ctypes.data, gap.ctypes.data, off.ctypes.data, flat.ctypes.data, kept.ctypes.data))
    return [flat[off[f]:off[f] + kept[f]].copy() for f in range(len(ns))]


def seg_gen_host(regs, anchors, qlens, hashes):
    """mm2gb_seg_gen_host (mm_seg_gen, hit.c:331-385): regs / anchors = per fragment its kept records (REG_DTYPE) and kept anchors ((m,2) uint64), qlens = per fragment
    its mate lengths, hashes = per fragment the hash mm_gen_regs gets.  Returns per fragment a list of (records, anchors) per mate."""
    ns, ql = _frag_arrays([len(q) for q in qlens], qlens)
    off = np.concatenate([[0], np.cumsum([len(r) for r in regs])]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(r, REG_DTYPE) for r in regs]) if len(regs) and off[-1] else np.zeros(0, REG_DTYPE))
    a_off = np.concatenate([[0], np.cumsum([len(a) for a in anchors])]).astype(np.int64)
    a = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint64).reshape(-1, 2) for x in anchors]) if len(anchors) and a_off[-1] else np.zeros((0, 2), np.uint64))
    hs = np.ascontiguousarray(hashes, dtype=np.uint32)
    o = SegOut()
    fn = lib().mm2gb_seg_gen_host
    fn.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SegOut)]
    _check(fn(len(ns), ns.ctypes.data, ql.ctypes.data, hs.ctypes.data, off.ctypes.data, flat.ctypes.data, a_off.ctypes.data, a.ctypes.data, C.byref(o)))
    U = 2 * len(ns)
    r_off, x_off = _take(o.reg_off, U + 1, np.int64), _take(o.anchor_off, U + 1, np.int64)
    r = _take(o.regs, int(r_off[-1]), REG_DTYPE) if U else np.zeros(0, REG_DTYPE)
    x = _take(o.anchors, int(x_off[-1]) * 2, np.uint64).reshape(-1, 2) if U else np.zeros((0, 2), np.uint64)
    lib().mm2gb_seg_out_free.argtypes = [C.POINTER(SegOut)]
    lib().mm2gb_seg_out_free.restype = None
    lib().mm2gb_seg_out_free(C.byref(o))
    return [[(r[r_off[2 * f + s]:r_off[2 * f + s + 1]], x[x_off[2 * f + s]:x_off[2 * f + s + 1]]) for s in range(int(ns[f]))] for f in range(len(ns))]


def _frags_args(frags, pe_ori):
    """The fragments' offsets as the C calls take them (the array is returned too: it must outlive the call)."""
    fo = np.ascontiguousarray(frags, dtype=np.int32)
    if len(fo) < 1:
        raise Mm2gbError("frags: frag_offsets(names), one more entry than fragments")
    return fo, (len(fo) - 1, fo.ctypes.data, int(pe_ori))


def map_reads(engine, index, ref_names, reads, opt=None, k=15, align=None, out=None, frags=None, pe_ori=1):
    """mm2gb_map_reads: reads = list of (name, sequence bytes); returns (PAF text, stats dict).  index: a SeedIndex of the references.
    frags (with align=map_sr(), opt=map_opt_sr()): frag_offsets(names) -- paired ends: mm2gb_map_frags_sr maps every run of two reads as one fragment (minimap2 -x sr
    r1.fq r2.fq without -c; interleave() makes the list from two files); pe_ori: mm_mapopt_t::pe_ori (1: the second mate is turned, the preset's).  None: single reads.
    align: a map_align(...) for base-level alignment (mm2gb_map_reads_aln) or a map_splice(...) for spliced reads (mm2gb_map_reads_splice); the stats then hold s_align, s_post_align and s_text as well.
    A map_sr(...) with opt=map_opt_sr(): short single-end reads (mm2gb_map_reads_sr; minimap2 -x sr [-c]); the stats then hold the call's own counts as well (n_chain_calls,
    n_rescued, n_tied_reads, sr_counts) and the three alignment seconds.
    out: a map_out(...) with any align= that aligns: SAM lines instead of PAF, = / X CIGARs (the calls named _out); None: the bytes of before."""
    _out_needs_align(out, align)
    L = lib()
    head = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_int32, C.c_void_p]
    tail = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p]
    L.mm2gb_map_reads.argtypes = head + tail
    L.mm2gb_map_reads_aln.argtypes = head + [C.POINTER(MapAln)] + tail + [C.c_void_p]
    L.mm2gb_map_reads_splice.argtypes = head + [C.POINTER(MapSplice)] + tail + [C.c_void_p]
    L.mm2gb_map_reads_sr.argtypes = head + [C.POINTER(MapSr)] + tail + [C.POINTER(MapSrOut)]
    L.mm2gb_map_reads_aln_out.argtypes = L.mm2gb_map_reads_aln.argtypes + [C.POINTER(MapOut)]
    L.mm2gb_map_reads_splice_out.argtypes = L.mm2gb_map_reads_splice.argtypes + [C.POINTER(MapOut)]
    L.mm2gb_map_reads_sr_out.argtypes = L.mm2gb_map_reads_sr.argtypes + [C.POINTER(MapOut)]
    last = () if out is None else (C.byref(out),)          # (`out` names the result pointer below)
    opt = opt or map_opt()
    rn = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
    names = (C.c_char_p * len(reads))(*[n.encode() for n, _ in reads])
    seqs_b = [bytes(s) for _, s in reads]
    seqs = (C.c_char_p * len(reads))(*seqs_b)
    lens = np.ascontiguousarray([len(s) for s in seqs_b], dtype=np.int32)
    out, n, st, extra = C.c_void_p(), C.c_int64(), MapStats(), (C.c_double * 3)()
    first = (engine._h, index._h, k, rn, index.lens.ctypes.data, len(ref_names), C.byref(opt))
    rest = (len(reads), names, seqs, lens.ctypes.data, C.byref(out), C.byref(n), C.byref(st))
    if frags is not None and not isinstance(align, MapSr):
        raise Mm2gbError("map_reads: frags= goes with align=map_sr() and opt=map_opt_sr() (paired ends are short reads)")
    if isinstance(align, MapSr):
        if align.align:
            _check_align_refs(align, ref_names)
        so = MapSrOut()
        if frags is not None:
            L.mm2gb_map_frags_sr.argtypes = L.mm2gb_map_reads_sr.argtypes + [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
            keep, more = _frags_args(frags, pe_ori)          # (keep: the offsets' array lives until the call returns)
            _check(L.mm2gb_map_frags_sr(*first, C.byref(align), *rest, C.byref(so), *more, last[0] if last else None))
        else:
            _check((L.mm2gb_map_reads_sr_out if last else L.mm2gb_map_reads_sr)(*first, C.byref(align), *rest, C.byref(so), *last))
        text = C.string_at(out, n.value).decode()
        L.mm2gb_free(out)
        return text, _sr_stats(st, so)
    if align is None:
        _check(L.mm2gb_map_reads(*first, *rest))
    else:
        _check_align_refs(align, ref_names)
        if not last:
            fn = L.mm2gb_map_reads_splice if isinstance(align, MapSplice) else L.mm2gb_map_reads_aln
        else:
            fn = L.mm2gb_map_reads_splice_out if isinstance(align, MapSplice) else L.mm2gb_map_reads_aln_out
        _check(fn(*first, C.byref(align), *rest, extra, *last))
    text = C.string_at(out, n.value).decode()
    L.mm2gb_free(out)
    return text, st.as_dict() if align is None else _stats_with_extra(st, extra)


def map_reads_multi(engines, index, ref_names, reads, opt=None, k=15):
    """mm2gb_map_reads_multi: like map_reads over a list of engines (one per device): reads shard, PAF in read order."""
    L = lib()
    L.mm2gb_map_reads_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                        C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p]
    opt = opt or map_opt()
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    rn = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
    names = (C.c_char_p * len(reads))(*[n.encode() for n, _ in reads])
    seqs_b = [bytes(s) for _, s in reads]
    seqs = (C.c_char_p * len(reads))(*seqs_b)
    lens = np.ascontiguousarray([len(s) for s in seqs_b], dtype=np.int32)
    out, n, st = C.c_void_p(), C.c_int64(), MapStats()
    _check(L.mm2gb_map_reads_multi(hs, len(engines), index._h, k, rn, index.lens.ctypes.data, len(ref_names), C.byref(opt), len(reads), names, seqs, lens.ctypes.data,
                                   C.byref(out), C.byref(n), C.byref(st)))
    text = C.string_at(out, n.value).decode()
    L.mm2gb_free(out)
    return text, st.as_dict()


def _engine_release_host_scratch(self):
    """Give back the large host arrays the engine's mapping / re-chaining calls keep between calls (mm2gb_engine_release_host_scratch)."""
    L = lib()
    L.mm2gb_engine_release_host_scratch.argtypes = [C.c_void_p]
    _check(L.mm2gb_engine_release_host_scratch(self._h))


Engine.release_host_scratch = _engine_release_host_scratch


def map_reads_stream(engines, index, ref_names, reads, opt=None, k=15, chunk_bases=0, align=None, out=None, frags=None, pe_ori=1):
    """mm2gb_map_reads_stream: a run of any size as a stream of chunks of about chunk_bases bases; every engine (several per device overlap
    host stages with kernels, engines on several devices shard the reads) takes the next chunk.  Returns (PAF text in read order, stats:
    counts summed, s_* summed over chunks).  align, out: as for map_reads (mm2gb_map_reads_stream_aln / _splice / _sr, and their _out forms).
    frags, pe_ori: as for map_reads (mm2gb_map_frags_stream_sr; a chunk ends between fragments)."""
    _out_needs_align(out, align)
    L = lib()
    head = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_int32, C.c_void_p]
    tail = [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p]
    L.mm2gb_map_reads_stream.argtypes = head + tail
    L.mm2gb_map_reads_stream_aln.argtypes = head + [C.POINTER(MapAln)] + tail + [C.c_void_p]
    L.mm2gb_map_reads_stream_splice.argtypes = head + [C.POINTER(MapSplice)] + tail + [C.c_void_p]
    L.mm2gb_map_reads_stream_sr.argtypes = head + [C.POINTER(MapSr)] + tail + [C.POINTER(MapSrOut)]
    L.mm2gb_map_reads_stream_aln_out.argtypes = L.mm2gb_map_reads_stream_aln.argtypes + [C.POINTER(MapOut)]
    L.mm2gb_map_reads_stream_splice_out.argtypes = L.mm2gb_map_reads_stream_splice.argtypes + [C.POINTER(MapOut)]
    L.mm2gb_map_reads_stream_sr_out.argtypes = L.mm2gb_map_reads_stream_sr.argtypes + [C.POINTER(MapOut)]
    last = () if out is None else (C.byref(out),)          # (`out` names the result pointer below)
    opt = opt or map_opt()
    hs = (C.c_void_p * len(engines))(*[e._h for e in engines])
    rn = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
    names = (C.c_char_p * len(reads))(*[n.encode() for n, _ in reads])
    seqs_b = [s if isinstance(s, bytes) else bytes(s) for _, s in reads]
    seqs = (C.c_char_p * len(reads))(*seqs_b)
    lens = np.ascontiguousarray([len(s) for s in seqs_b], dtype=np.int32)
    out, n, st, extra = C.c_void_p(), C.c_int64(), MapStats(), (C.c_double * 3)()
    first = (hs, len(engines), index._h, k, rn, index.lens.ctypes.data, len(ref_names), C.byref(opt))
    rest = (len(reads), names, seqs, lens.ctypes.data, int(chunk_bases), C.byref(out), C.byref(n), C.byref(st))
    if frags is not None and not isinstance(align, MapSr):
        raise Mm2gbError("map_reads_stream: frags= goes with align=map_sr() and opt=map_opt_sr() (paired ends are short reads)")
    if isinstance(align, MapSr):
        if align.align:
            _check_align_refs(align, ref_names)
        so = MapSrOut()
        if frags is not None:
            L.mm2gb_map_frags_stream_sr.argtypes = L.mm2gb_map_reads_stream_sr.argtypes + [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
            keep, more = _frags_args(frags, pe_ori)          # (keep: the offsets' array lives until the call returns)
            _check(L.mm2gb_map_frags_stream_sr(*first, C.byref(align), *rest, C.byref(so), *more, last[0] if last else None))
        else:
            _check((L.mm2gb_map_reads_stream_sr_out if last else L.mm2gb_map_reads_stream_sr)(*first, C.byref(align), *rest, C.byref(so), *last))
        text = C.string_at(out, n.value).decode()
        L.mm2gb_free(out)
        return text, _sr_stats(st, so)
    if align is None:
        _check(L.mm2gb_map_reads_stream(*first, *rest))
    else:
        _check_align_refs(align, ref_names)
        if not last:
            fn = L.mm2gb_map_reads_stream_splice if isinstance(align, MapSplice) else L.mm2gb_map_reads_stream_aln
        else:
            fn = L.mm2gb_map_reads_stream_splice_out if isinstance(align, MapSplice) else L.mm2gb_map_reads_stream_aln_out
        _check(fn(*first, C.byref(align), *rest, extra, *last))
    text = C.string_at(out, n.value).decode()
    L.mm2gb_free(out)
    return text, st.as_dict() if align is None else _stats_with_extra(st, extra)
