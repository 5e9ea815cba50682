"""Adaptive sampling on the CPU (pt_api.h: pt_render_adaptive): the numpy
restatement of its batch loop (tests/adaptive_model.py) on the oracle's Cornell frames, guarding
the inputs tests/test_gpu_adaptive.py depends on, and the per-tile stop rule of csrc/pt_noise.h
through its host entry point against numpy.  No device is touched."""
from collections import Counter

import numpy as np
import pytest

import adaptive_model as M
import oracle_lib as O
import pt_host as H
from test_noise_host import q_numpy

f32 = np.float32
W, HH, B = 64, 48, 8


@pytest.fixture(scope="module")
def cornell64(cornell_scene):
    return [O.render(cornell_scene, W, HH, max_bounce=B, frame_first=f, n_frames=1, acc_first=0) for f in range(1, 65)]


def test_cornell_tiles_retire_at_different_batches(cornell64):
    """Cornell 64 x 48, frames 1..64 in batches of 8, target 0.25, 8 x 8 tiles: the spread of
    per-tile frame counts the GPU cases need, and the distribution the feature was proposed on."""
    r = M.run(cornell64, W, HH, 0, 8, 64, 0.25)
    counts = Counter(int(f) for f in r["frames"].reshape(-1))
    print("tiles per frame count:", sorted(counts.items()), r["stats"])
    assert len(counts) >= 4
    assert counts[8] >= 1                                   # a tile retires after the first batch
    assert r["stats"]["tiles_active"] >= 1                  # a tile is still active at max_frames
    assert any(8 < f < 64 for f in counts)                  # a tile retires exactly at a middle batch
    assert counts == {8: 12, 16: 5, 24: 5, 32: 3, 48: 1, 56: 2, 64: 20}
    assert r["stats"]["tiles"] == 48 and r["stats"]["tiles_active"] == 19
    assert r["stats"]["pixel_frames"] == 117248 and r["frames_done"] == 64
    assert r["stats"]["pixels"] == W * HH and r["stats"]["frames"] == 64


def test_model_edges(cornell64):
    """Everything retires after one batch for a target of 64, nothing for 1e-6; a footprint
    leaves tiles without a pixel at 0 frames; a short last batch."""
    r = M.run(cornell64, W, HH, 0, 8, 64, 64.0)
    assert r["frames_done"] == 8 and (r["frames"] == 8).all() and r["stats"]["tiles_active"] == 0
    r = M.run(cornell64, W, HH, 0, 8, 60, 1e-6)
    assert r["frames_done"] == 60 and (r["frames"] == 60).all() and r["stats"]["tiles_active"] == 48
    mask = np.zeros((HH, W), np.uint8)
    mask[:40, :60] = 1
    r = M.run(cornell64, W, HH, 0, 8, 64, 0.25, mask=mask)
    assert (r["frames"][5] == 0).all() and (r["frames"][:5] > 0).all() and r["stats"]["tiles"] == 40
    assert r["stats"]["pixels"] == 2400 and (r["pixel_frames"][:, 60:] == 0).all()


def rule_numpy(s1, s2, n, target, mask=None):
    q = q_numpy(s1, s2, n).astype(np.uint64).reshape(-1)
    if mask is not None:
        q = q[np.asarray(mask).reshape(-1) != 0]
    return int(q.sum()) <= M.target_q(target) * q.size


@pytest.mark.parametrize("pixels", [1, 7, 64])
def test_tile_rule_matches_numpy(pixels):
    """ptn::tile_retires through pt_tile_retires_host on random tiles whose mean relative error
    straddles the target: both verdicts occur, and each equals numpy's."""
    rng = np.random.default_rng(50 + pixels)
    seen = set()
    for _ in range(300):
        n = int(rng.integers(2, 200))
        mean = np.exp2(rng.uniform(-6, 3, pixels)).astype(f32)
        rel_var = np.exp2(rng.uniform(-8, 6)) * rng.uniform(0.5, 2.0, pixels)
        s1 = (mean * f32(n)).astype(f32)
        s2 = (f32(n) * mean * mean * (1.0 + rel_var).astype(f32)).astype(f32)
        mask = None if rng.random() < 0.5 else (rng.random(pixels) < 0.7).astype(np.uint8)
        target = float(np.exp2(rng.uniform(-5, 1)))
        want = rule_numpy(s1, s2, n, target, mask)
        assert H.tile_retires_host(np.stack([s1, s2], -1), n, target, mask) == want
        seen.add(want)
    assert seen == {True, False}


def test_tile_rule_edges():
    nan = f32(np.nan)
    # a NaN pixel has q = 64 * 65536: its one-pixel tile never retires for a target below 64 ...
    assert q_numpy([nan], [1.0], 8)[0] == 64 << 16
    assert not H.tile_retires_host(np.array([[nan, 1.0]], f32), 8, 0.999)
    assert H.tile_retires_host(np.array([[nan, 1.0]], f32), 8, 64.0)
    # ... and among 63 black pixels (q = 0) the tile's mean is 64 / 64 = 1: it retires at 1, not below
    mom = np.zeros((64, 2), f32)
    mom[17] = (nan, nan)
    assert H.tile_retires_host(mom, 16, 1.0) and not H.tile_retires_host(mom, 16, 0.999)
    assert rule_numpy(mom[:, 0], mom[:, 1], 16, 1.0) and not rule_numpy(mom[:, 0], mom[:, 1], 16, 0.999)
    # the sum lands exactly on target_q * pixels: retires (<=); one step of the target lower: stays
    s1, s2 = np.array([4.0, 4.0], f32), np.array([10.0, 10.0], f32)
    q = int(q_numpy(s1, s2, 2)[0])
    assert H.tile_retires_host(np.stack([s1, s2], -1), 2, q / 65536.0)
    assert not H.tile_retires_host(np.stack([s1, s2], -1), 2, (q - 1) / 65536.0)
    # a one-pixel tile, and pixels outside the footprint are not seen
    assert H.tile_retires_host(np.array([[0.0, 0.0]], f32), 2, 0.01)
    assert H.tile_retires_host(np.array([[0.0, 0.0], [nan, nan]], f32), 2, 0.01, [1, 0])
    for n in (0, 1):
        with pytest.raises(H.PTError):
            H.tile_retires_host(np.zeros((4, 2), f32), n, 0.25)
