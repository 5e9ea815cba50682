"""The per-pixel noise estimate on the host (pt_api.h: pt_noise_host; csrc/pt_noise.h, the
functions the device kernels run) against a numpy float32 restatement of its definition, bit
for bit: every operation is a separately rounded binary32 operation, so there is no tolerance.
No device is touched."""
import numpy as np
import pytest

import pt_host as H

f32 = np.float32


def q_numpy(s1, s2, n):
    """(S1, S2, n) -> q, the definition in pt_api.h restated in numpy float32."""
    s1, s2 = np.asarray(s1, f32), np.asarray(s2, f32)
    with np.errstate(all="ignore"):
        nf = f32(n)
        m = s1 / nf
        v = np.maximum(s2 / nf - m * m, f32(0.0))
        sem = np.sqrt(v / f32(n - 1))
        rel = sem / (m + f32(0.01))
        rel = np.where(rel <= f32(64.0), rel, f32(64.0)).astype(f32)
        return (rel * f32(65536.0)).astype(np.uint32)


def stats_numpy(s1, s2, n, target, mask=None):
    q = q_numpy(s1, s2, n).astype(np.uint64).reshape(-1)
    if mask is not None:
        q = q[np.asarray(mask).reshape(-1) != 0]
    tq = np.uint64(int(f32(target) * f32(65536.0)))
    return dict(pixels=int(q.size), sum_q=int(q.sum()), above=int(np.count_nonzero(q > tq)),
                max_q=int(q.max()) if q.size else 0, frames=n)


def check(s1, s2, n, target, mask=None):
    mom = np.stack([np.asarray(s1, f32), np.asarray(s2, f32)], axis=-1)
    got = H.noise_host(mom, n, target, mask)
    want = stats_numpy(s1, s2, n, target, mask)
    assert {k: got[k] for k in want} == want
    return got


def per_pixel(s1, s2, n):
    """q of single pixels through the library (a one-pixel summary's max_q)."""
    return np.array([H.noise_host(np.array([a, b], f32), n, 1.0)["max_q"] for a, b in zip(s1, s2)], np.uint32)


@pytest.mark.parametrize("n", [2, 3, 37, 1024])
def test_random_moments_match_numpy_bitwise(n):
    """4,096 random (S1, S2) pairs per frame count: sums of n luminances whose mean spans
    2^-12..2^6 and whose variance spans zero (S2/n just below m^2: the clamp) to many times
    the mean; q pixel by pixel and the summary's fields."""
    rng = np.random.default_rng(1000 + n)
    mean = np.exp2(rng.uniform(-12, 6, 4096)).astype(f32)
    rel_var = np.where(rng.random(4096) < 0.25, rng.uniform(-1e-6, 1e-6, 4096), np.exp2(rng.uniform(-20, 8, 4096)))
    s1 = (mean * f32(n)).astype(f32)
    s2 = (f32(n) * mean * mean * (1.0 + rel_var).astype(f32)).astype(f32)
    want_q = q_numpy(s1, s2, n)
    assert np.array_equal(per_pixel(s1[:512], s2[:512], n), want_q[:512])
    assert len(np.unique(want_q)) > 1000 and want_q.min() == 0    # the clamp to zero variance is hit
    got = check(s1, s2, n, 0.25)
    assert 0 < got["above"] < got["pixels"] == 4096


def test_edge_cases():
    inf, nan = f32(np.inf), f32(np.nan)
    # S1 = S2 = 0: a black pixel is converged
    assert per_pixel([0.0], [0.0], 2)[0] == 0
    # S2/n < m^2 by rounding: the variance clamps to 0
    s1, s2 = f32(3.0), f32(np.nextafter(f32(4.5), f32(0)))
    assert s2 / f32(2) < (s1 / f32(2)) * (s1 / f32(2)) and per_pixel([s1], [s2], 2)[0] == 0
    # NaN and infinite moments count as the largest relative error, 64
    bad1 = [nan, 1.0, nan, inf, -inf, 1.0]
    bad2 = [1.0, nan, nan, inf, inf, inf]
    for n in (2, 16):
        assert np.array_equal(per_pixel(bad1, bad2, n), np.full(6, 64 << 16, np.uint32))
        assert np.array_equal(q_numpy(bad1, bad2, n), np.full(6, 64 << 16, np.uint32))
    # a huge variance over a tiny mean clamps to 64 too
    assert per_pixel([1e-6], [1e6], 4)[0] == 64 << 16 == q_numpy([1e-6], [1e6], 4)[0]
    # n = 2: the smallest count; two samples 1 and 3: m = 2, v = 1, sem = 1, rel = 1 / 2.01
    assert per_pixel([4.0], [10.0], 2)[0] == q_numpy([4.0], [10.0], 2)[0] == int(f32(1.0) / f32(2.01) * f32(65536.0))
    # a mean at or below -0.01 (no render produces one) has no relative error: counted as 64
    assert per_pixel([-1.0], [1.0], 2)[0] == 64 << 16
    for n in (0, 1, -3):
        with pytest.raises(H.PTError):
            H.noise_host(np.zeros((4, 2), f32), n, 0.25)


def test_target_on_a_q_and_summary_fields():
    rng = np.random.default_rng(7)
    s1 = rng.uniform(0.5, 40.0, 300).astype(f32)
    s2 = (s1 * s1 / f32(8) * rng.uniform(1.0, 3.0, 300).astype(f32)).astype(f32)
    q = q_numpy(s1, s2, 8)
    pick = int(np.sort(q)[150])
    assert 0 < pick < 64 << 16
    # q / 65536 is exact in binary32 (q <= 2^22): the target lands exactly on that pixel's q,
    # which is then not above it; one step lower it is
    on = check(s1, s2, 8, pick / 65536.0)
    below = check(s1, s2, 8, (pick - 1) / 65536.0)
    assert on["above"] == int(np.count_nonzero(q > pick))
    assert below["above"] == int(np.count_nonzero(q >= pick)) > on["above"]
    assert on["mean"] == on["sum_q"] / 300 / 65536.0 and on["max"] == int(q.max()) / 65536.0


def test_footprint_mask():
    rng = np.random.default_rng(8)
    s1 = rng.uniform(0.5, 40.0, (12, 17)).astype(f32)
    s2 = (s1 * s1 / f32(5) * rng.uniform(1.0, 2.0, (12, 17)).astype(f32)).astype(f32)
    mask = np.zeros((12, 17), np.uint8)
    mask[:10, :10] = 1
    s2[11, 16] = np.nan                      # outside the footprint: must not be seen
    got = check(s1, s2, 5, 0.1, mask)
    assert got["pixels"] == 100 and got["max_q"] < 64 << 16
    assert check(s1, s2, 5, 0.1)["max_q"] == 64 << 16
    none = check(s1, s2, 5, 0.1, np.zeros((12, 17), np.uint8))
    assert none == dict(none, pixels=0, sum_q=0, above=0, max_q=0)
