"""What the GPU tests of the planner's sparse list rest on, checked without a device: the numpy model of the planner's rule
(test_gpu_sparse_fill.expected_sparse) on the batches of clamped windows beside sparse chunks, the oracle's rescue links in them, and
the share of the soak's fuzz batches that hold a chunk for the list at all."""
import numpy as np
import pytest

import orc
import synth_cases as sc
from test_gpu_parity import fuzz_seed, rel
from test_gpu_sparse_fill import CLAMP_CASES, NO_GANGS, TEAM_ENVS, clamp_batch, clamp_conditions, expected_sparse, heavy_rule


@pytest.mark.parametrize("max_iter,n_noise", CLAMP_CASES)
def test_clamp_batches_test_the_flag(max_iter, n_noise):
    """clamp_conditions' assertions (the rescue reads are narrow enough for the list and clamped; some chunks stay on the list, some
    leave it; the inclusive block count differs from a chunk's own block), and in every rescue read a link longer than max_iter"""
    a, off, rescue_reads = clamp_batch(n_noise)
    counts = {clamp_conditions(a, off, rescue_reads, max_iter, n_noise, heavy_rule(env)) for env in (NO_GANGS, TEAM_ENVS["teams-of-4"])}
    assert len(counts) == 1                                         # nothing in the batch is heavy under either engine
    _, po, _ = orc.chain_fill_many(a, off, orc.default_param(max_iter=max_iter), threads=2)
    for r in rescue_reads:
        assert max_iter >= n_noise or rel(po[off[r]:off[r + 1]]).max() > max_iter


def test_the_soak_batches_hold_chunks_for_the_list():
    """the first 100 batches of fuzz_soak.py's seed in the suite: at least a fifth have a chunk the planner would send to the sparse list"""
    rng = np.random.default_rng(fuzz_seed() ^ 0x5eed)
    with_list = 0
    for _ in range(100):
        a, off, kw = sc.fuzz_case(rng)
        with_list += len(a) > 0 and expected_sparse(a, off, orc.default_param(**kw), heavy=heavy_rule({})) > 0
    assert with_list >= 20, with_list
