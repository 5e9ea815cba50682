"""Cameras and reference models of the camera-model tests (tests/test_camera_host.py on the CPU, tests/test_gpu_camera.py
on the GPU).  The scenes are tests/query_cases.py's, the seeded cameras tests/trace_cases.py's.

rng_draws(): the camera's draws from Python integers (the reference's hash, computeShader.c:87-98), independent of any
product code.  model_ray(): the four models in float64 numpy, written from the real-number definitions of
include/pt_api.h, not from csrc/pt_camera.h: the basis from the camera's 12 floats, u and v by a plain division, the
library's sin and cos.  It shares with the product only the constant 3.1415926f (part of the definition) and the
binary32 values of the draws.
"""
import numpy as np

import pt_host as H

f32 = np.float32
MODELS = ["pinhole", "thinlens", "ortho", "equirect"]
N_DRAWS = {("pinhole", True): 2, ("pinhole", False): 0, ("thinlens", True): 4, ("thinlens", False): 2,
           ("ortho", True): 2, ("ortho", False): 0, ("equirect", True): 2, ("equirect", False): 0}
PI = float(f32(3.1415926))          # the definition's constant, as binary32 holds it
M32 = 0xFFFFFFFF


def camera(model, W, Hh, cam, aa=True, aperture=0.05, focus=6.0, ortho_width=4.0):
    return H.Camera(model, W, Hh, cam, aperture=aperture, focus=focus, ortho_width=ortho_width, aa=aa)


def py_seed(x, y, frame):
    return (y * 831266 + x * 923766 + frame * 719393) & M32


def py_next_random(s):
    s = (s * 747796405 + 2891336453) & M32
    r = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & M32
    return s, ((r >> 22) ^ r) & M32


def rng_draws(x, y, frame, n):
    """-> (the n random01 values as float64 of their binary32 values, the state after them)."""
    s = py_seed(int(x), int(y), int(frame))
    out = []
    for _ in range(n):
        s, r = py_next_random(s)
        out.append(float(f32(f32(r) * f32(2.0 ** -32))))
    return out, s


def states_after(xy, frame, n):
    return np.array([rng_draws(x, y, frame, n)[1] for x, y in xy], np.uint32)


def _unit(v):
    return v / np.linalg.norm(v)


def basis64(c):
    cam = np.array(list(c.cam), np.float64)
    pos, fwd = cam[0:3], _unit(cam[4:7])
    right = _unit(np.cross(fwd, [0.0, 0.0, 1.0]))
    upU = _unit(np.cross(right, fwd))
    return pos, fwd, right, upU, upU * c.height / c.width


def model_ray(c, x, y, draws, basis=None, duv=0.0):
    """The float64 ray of pixel (x, y) of Camera c from the draws [ax, ay, u1, u2] (those the model and flags take,
    in order) -> dict(o, d, P): P is the thin lens's point in focus, else None.  duv: added to u and v (the conditioning
    checks move them by a rounding of binary32 at 0.5)."""
    pos, fwd, right, upU, upS = basis if basis is not None else basis64(c)
    draws = list(draws)
    ax, ay = (draws.pop(0), draws.pop(0)) if not (c.flags & H.PT_CAM_NO_AA) else (0.0, 0.0)
    u, v = (x + ax) / c.width - 0.5 + duv, (y + ay) / c.height - 0.5 + duv
    P = None
    if c.model == H.PT_CAM_PINHOLE:
        o, d = pos, _unit(fwd + right * u + upS * v)
    elif c.model == H.PT_CAM_THIN_LENS:
        u1, u2 = draws
        D = fwd + right * u + upS * v
        P = pos + D * float(c.focus)
        r, phi = float(c.aperture) * np.sqrt(u1), 2.0 * PI * u2
        o = pos + right * (r * np.cos(phi)) + upU * (r * np.sin(phi))
        d = _unit(P - o)
    elif c.model == H.PT_CAM_ORTHO:
        o, d = pos + right * (u * float(c.ortho_width)) + upS * (v * float(c.ortho_width)), fwd
    else:
        theta, alpha = 2.0 * PI * (u + 0.5), PI * (v + 0.5)
        F = _unit(np.array([fwd[0], fwd[1], 0.0]))
        h = F * -np.cos(theta) + right * -np.sin(theta)
        o, d = pos, _unit(h * np.sin(alpha) + np.array([0.0, 0.0, -np.cos(alpha)]))
    return dict(o=np.asarray(o, np.float64), d=np.asarray(d, np.float64), P=P)


def normalize32(v):
    """pt::normalize in numpy binary32: (x x + y y) + z z, then v * (1 / sqrt(q)), every step rounded once."""
    v = np.asarray(v, f32)
    q = f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))
    return (v * f32(f32(1.0) / np.sqrt(q))).astype(f32)


def ray_words(rays):
    return np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 8)
