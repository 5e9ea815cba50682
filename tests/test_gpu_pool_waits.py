"""The pipelined leaf sweep of k_render_pool (ptc::sweep_mask_piped on the LDS copy of the sweep table; DESIGN.md
§5.12, "Round 16") on the GPU.  Every case renders the oracle's words with the pool on and with it off, as
tests/test_gpu_path_pool.py does, at the table sizes at which the chunked loop takes another path;
tests/test_pool_waits.py holds the CPU side.  (The round's other two parts, a cached run of tile positions per queue
reservation and an early request of the leaf re-test's box, did not pay and are not in the kernel; the pool suite
already covers the shapes they would have needed.)
"""
import os
import re

import pytest

from test_gpu_path_pool import both
from test_leaf_sweep import CSRC, SWEEP_MAX_LEAVES, quad_rows, scene_with_leaves

pytestmark = pytest.mark.gpu


def kernel_depth():
    text = open(os.path.join(CSRC, "pt_render_pool.h")).read()
    return int(re.search(r"#ifndef PT_POOL_SWEEP_DEPTH\s*\n#define PT_POOL_SWEEP_DEPTH (\d+)", text).group(1))


D = max(kernel_depth(), 1)


@pytest.mark.parametrize("leaves", sorted({2, 3, D, D + 1, 2 * D, 2 * D + 1, 3 * D, 3 * D + 1, 4 * D, SWEEP_MAX_LEAVES} - {0, 1}))
def test_sweep_table_sizes(leaves):
    """The chunked loop's paths: fewer boxes than a chunk (the plain remainder only), one chunk, one chunk and a
    remainder, two chunks (no trip of the unrolled loop), one trip of it with nothing, a remainder and one more chunk
    after it, and the largest table."""
    both(scene_with_leaves(leaves), "%d leaves" % leaves, 32, 24)


def test_waves_that_skip_the_sweep():
    """The camera stands outside the root box: whole waves skip the sweep on the root's own test."""
    both(quad_rows(11), "11 quads seen from outside their box", 32, 24)
