"""Named triangle lists for the BVH builders' edge cases (tests/test_bvh_cases.py on the CPU,
tests/test_gpu_bvh.py on the GPU).  Deterministic, numpy only; every case is (n, 16) float32 in
the reference's std140 triangle records.

The GPU builder (csrc/pt_bvh_gpu.hip) promises the host builder's nodes word for word, and that
rests on four order-sensitive rules:
  union      the box union keeps the left operand unless the right one is strictly smaller /
             larger (associative, not commutative: which of -0 / +0 a bound keeps);
  cost       the first minimum under strict `<` wins among the split candidates;
  zero       -0 == +0 in the centroid key;
  stability  the centroid sorts are stable.
The device runs them in hipcub primitives whose tiles are 1,024 items here (rocPRIM's default
configurations for gfx950, read from its headers: scan-by-key of an int key with the 24-byte box
is 256 threads x 4 items; the radix sort of 64-bit keys with int values is one 256 x 4 block up to
1,024 items, a merge sort over 1,024-item block sorts up to 2^20 items, and one-sweep passes of
512 x 16 items only above that).  Every multi-tile case below has at least four tiles, so the
scans' cross-tile look-back, the sort's block merges and segment boundaries inside a tile all
take part.

Sensitivity record.  Each rule was broken in a scratch copy of the host builder, one at a time
(`<=` in grow(), `<=` in the cost compare, a centroid compare that puts -0 before +0,
std::sort for std::stable_sort); a case is listed under a rule when the broken builder's nodes
differ from the unbroken builder's:

  case                       n  tiles  union  cost  zero  stability
  plane                 20,000  19.5    x      x     -     x
  lattice               21,952  21.4    -      x     -     x
  identical             20,000  19.5    x      -     x     x
  flat_ints              6,000   5.9    x      x     x     x
  subnormal_1e-41        3,000   2.9    -      x     -     x
  large_1e37             3,000   2.9    -      x     -     -
  overflow_3.3e38          500   0.5    -      -     -     x
  chain120_2.0, chain200_1.3 (forward)  -      -     -     -
  chain120_2.0_rev, chain200_1.3_rev    -      x     -     -
  soup59 .. soup180                     -      x     -     -
  (the earlier 40 flat quads, one tile) x      x     x     x
Every rule is noticed by at least one case of four tiles or more.

CASES maps a name to a function returning the triangles; get(name) caches the array (read-only).
"""
import functools

import numpy as np

SCAN_TILE = 1024        # items per hipcub scan-by-key / block-sort tile (see above)


def _tris(v0, v1, v2, mat=None):
    n = len(v0)
    t = np.zeros((n, 16), np.float32)
    t[:, 0:3], t[:, 4:7], t[:, 8:11] = v0, v1, v2
    if mat is not None:
        t[:, 12] = mat
    return t


# ------------------------------------------------------------------ multi-tile tie cases
def plane():
    """A 100 x 100 grid of unit cells in z = 0, two triangles per cell, the cell's z written as
    -0.0 or +0.0 by cell parity: every box is flat, centroids tie along rows and columns, and
    which zero a bound keeps depends on the union's order."""
    i, j = np.meshgrid(np.arange(100), np.arange(100), indexing="ij")
    i, j = i.reshape(-1).astype(np.float32), j.reshape(-1).astype(np.float32)
    z = np.where((i + j) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    p00, p10 = np.stack([i, j, z], 1), np.stack([i + 1, j, z], 1)
    p11, p01 = np.stack([i + 1, j + 1, z], 1), np.stack([i, j + 1, z], 1)
    a, b = _tris(p00, p10, p11), _tris(p00, p11, p01)
    t = np.empty((2 * len(a), 16), np.float32)
    t[0::2], t[1::2] = a, b
    return t


def lattice():
    """One small triangle repeated on a 28^3 integer lattice (21,952 triangles).  Its box is a
    cube and its centroid sum is the same on the three axes, so split costs tie exactly between
    axes and between mirrored candidates, and whole lattice planes tie in every centroid sort."""
    g = np.arange(28, dtype=np.float32)
    x, y, z = (a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij"))
    o = np.stack([x, y, z], 1)
    q = np.float32(0.25)
    return _tris(o + [0, 0, q], o + [q, 0, 0], o + [0, q, 0], np.arange(len(o)) % 5)


def identical():
    """20,000 copies of one degenerate triangle, every third with x = -0.0, materials cycling:
    nothing but the stable order decides, every cost is NaN (zero area: the median fallback), and
    the leaf indices go through the first-equal map."""
    n = 20000
    v = np.tile(np.array([0.0, 1.0, 2.0], np.float32), (n, 1))
    v[::3, 0] = -0.0
    return _tris(v, v, v, np.arange(n) % 7)


def flat_ints(n=6000):
    """Flat quads in z = 0 with small integer x, y (centroid ties, shared boxes) and z = -0.0 on
    the even rows.  Triangles that share a box tie at every split and peel off one at a time:
    the host tree is over 2,000 levels deep."""
    rng = np.random.default_rng(5)
    q = np.zeros((n, 16), np.float32)
    q[:, [0, 1, 4, 5, 8, 9]] = rng.integers(-3, 4, (n, 6)).astype(np.float32)
    q[::2, [2, 6, 10]] = -0.0
    return q


# ------------------------------------------------------------------ unbalanced trees
def chain(n, r, rev):
    """Triangle i at x = r^i (rev: -r^i) with size 0.1 r^i: the SAH peels the far triangles off
    one or a few at a time.  Forward, the right children finish first and the builder's processed
    window shrinks; reversed, the left children finish first and the window's start moves up."""
    x = np.float64(r) ** np.arange(n)
    s = 0.1 * x
    if rev:
        x = -x - s
    z = np.zeros(n)
    return _tris(np.stack([x, z, z], 1), np.stack([x + s, s, z], 1), np.stack([x, s, s], 1), np.arange(n) % 3)


# ------------------------------------------------------------------ magnitudes
def uniform_soup(n, scale, seed):
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1.0, 1.0, (n, 9)) * scale).astype(np.float32)
    return _tris(v[:, 0:3], v[:, 3:6], v[:, 6:9], rng.integers(0, 4, n))


# ------------------------------------------------------------------ sizes around the candidate stride
def gaussian_soup(n):
    """The soup of test_sizes_and_duplicates: a duplicate and two integer-coordinate triangles."""
    rng = np.random.default_rng(n)
    t = np.zeros((n, 16), np.float32)
    t[:, :12] = rng.normal(size=(n, 12)).astype(np.float32)
    t[:, [3, 7, 11]] = 0
    t[:, 12] = rng.integers(0, 4, n)
    if n >= 4:
        t[n // 2] = t[0]
        t[1, :12] = np.round(t[1, :12])
        t[2, :12] = np.round(t[2, :12])
    return t


MULTI_TILE = ["plane", "lattice", "identical", "flat_ints"]
# name -> (n, r, rev); the host tree's depth must be at least n / 8
CHAINS = {"chain120_2.0": (120, 2.0, False), "chain120_2.0_rev": (120, 2.0, True),
          "chain200_1.3": (200, 1.3, False), "chain200_1.3_rev": (200, 1.3, True)}
MAGNITUDES = ["subnormal_1e-41", "large_1e37", "overflow_3.3e38"]
STRIDE_SIZES = [59, 60, 119, 120, 179, 180]      # the candidate stride m / 60 + 1 changes at 60, 120, 180

CASES = {"plane": plane, "lattice": lattice, "identical": identical, "flat_ints": flat_ints,
         "subnormal_1e-41": functools.partial(uniform_soup, 3000, 1e-41, 41),
         "large_1e37": functools.partial(uniform_soup, 3000, 1e37, 37),
         "overflow_3.3e38": functools.partial(uniform_soup, 500, 3.3e38, 38)}
for _name, _args in CHAINS.items():
    CASES[_name] = functools.partial(chain, *_args)
for _n in STRIDE_SIZES:
    CASES["soup%d" % _n] = functools.partial(gaussian_soup, _n)


@functools.lru_cache(maxsize=None)
def get(name):
    t = np.ascontiguousarray(CASES[name](), np.float32)
    t.setflags(write=False)
    return t


def tree_depth(nodes):
    """Depth of a threaded tree (the root at depth 0) and its leaf count, from the hit / miss links: an
    internal node's hit link is its left child, whose miss link is the right child."""
    nodes = np.asarray(nodes, np.float32)
    depth, leaves, stack = 0, 0, [(0, 0)]
    while stack:
        i, d = stack.pop()
        depth = max(depth, d)
        if nodes[i, 8] > -1.0:
            leaves += 1
            continue
        left = int(nodes[i, 10])
        stack.append((int(nodes[left, 11]), d + 1))
        stack.append((left, d + 1))
    return depth, leaves
