"""The scheduler (csrc/sched.hpp and its consumers sched_kernel of csrc/elementwise.hpp and slot_sched_kernel of csrc/slots.hpp): a
host model of the Philox4x32-10 / Box-Muller noise, word for word what philox_normal4 and sched_noise4 feed the generator, with a
defect= switch; the three update forms and the CFG mix in unfused fp32 torch in the kernel's order, with rounding-count bounds
against the same expression in fp64; the tail seeds; the per-element noise tolerance; and the case lists shared by
tests/test_sched_noise_cpu.py and tests/test_sched_noise_gpu.py.  Plain helper module (pytest does not collect it), host only.

The noise
---------
  counter = (quad, step k, clip word, 0), key = (seed & 0xffffffff, seed >> 32); for flat element e of a buffer of clips of
  n_per_clip elements: clip = e // n_per_clip, quad = (e - clip * n_per_clip) >> 2, clip word = clip0 + clip (mod 2^32).
  r0..r3 = Philox4x32-10(counter, key).  In fp32, every operation rounding:
      u0 = min((f32(r0) + 0.5) * 2^-32, 1), u2 likewise from r2 (the log arguments), u1 = f32(r1) * 2^-32, u3 from r3 (turns)
  then ra = sqrt(-2 ln u0), rb = sqrt(-2 ln u2), z = (ra cos 2 pi u1, ra sin 2 pi u1, rb cos 2 pi u3, rb sin 2 pi u3).
  f32(r) rounds to nearest even: the top 128 values of r0 give 2^32, u0 = 1 and ra = 0; the smallest u0 is 2^-33, ra = 6.77.
  The model takes the fp32 uniforms exactly as the kernel forms them and does everything after them in fp64.

The tolerance
-------------
u = 2^-24.  After the (exact, shared) fp32 uniforms the kernel rounds:
  L = v_log_f32(u0)            the hardware log2, 1 ulp: relative 2u
  m = -1.3862943611198906f * L the constant is 2 ln 2 rounded to fp32 (u), the product rounds (u): m relative 4u
  ra = sqrtf(m)                halves the relative error of m (2u), its own correctly rounded result adds u: 3u
  z = ra * c                   the product rounds: u.  With c exact, z is relative 4u.
  c = v_cos_f32 / v_sin_f32(u1) on an exact fp32 angle in turns: an ABSOLUTE error E_TRIG, which reaches z as ra * E_TRIG.
      |z_gpu - z_ref| <= ra * E_TRIG + |z_ref| * E_REL + tiny,    E_REL = 2 * 4u, tiny = 1e-30
  The factor 2 in E_REL pays, as in tests/norm_cases.py, for the second-order products and for a 1-ulp instead of half-ulp sqrtf.
  E_TRIG is the one number that is measured, not counted: see the constant.  NOISE_ERR_CONDITION = 1e-4 is a condition, not a
  measurement: a worst |z_gpu - z_ref| above it is a finding whatever E_TRIG says (far above a 1-ulp-class log / trig unit, far
  below the O(1) change of any defect twin).

The updates
-----------
  mix      x0 = u + s (x0 - u)                                              3 roundings
  mode 0   o = c1 x0 + c2 x (+ sg z if t > 0)                               3 roundings, 5 with the noise
  mode 1   eps = (sra x - x0) / srm1; o = x0 san + cn eps                   6 roundings
  mode 3   o = b x0 + a x (+ c h if c != 0) (+ s z if s != 0)               3, +2 per optional term
  R roundings over terms whose magnitudes sum to A: |fp32 - fp64| <= gamma_R A, gamma_R = R u / (1 - R u).  The mix's own
  bound, times the magnitude of the coefficient x0 meets, is added when the mix runs in front.
"""
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
# the three published known-answer vectors of Philox4x32-10 (Random123 kat_vectors): (counter, key, output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

E_REL = 8.0 * U
# Measured on an MI355X by tests/test_sched_noise_gpu.py (test_noise_worst_is_reported, pytest -s) against the fp64 model below over
# the cases of section A (NOISE_CASES, the grid-stride buffers included) and the slots of B: the largest |z_gpu - z_ref| / ra, the
# whole difference attributed to the sine / cosine.  It read 2.2675e-07 (the worst |z_gpu - z_ref| itself 6.51e-07, in the
# grid-stride buffer; the worst element stood at 1.59 x the counted |z| E_REL term alone).  E_TRIG = 4 x that value: margin for angles
# the cases do not hit.  With it the largest tolerance the formula can give, at ra = 6.77, is 9.4e-06: a tenth of the condition.
E_TRIG_MEASURED = 2.27e-7
E_TRIG_MARGIN = 4.0
E_TRIG = E_TRIG_MARGIN * E_TRIG_MEASURED
NOISE_ERR_CONDITION = 1e-4
NOISE_TINY = 1e-30
RA_MAX = float(np.sqrt(2.0 * np.log(2.0 ** 33)))      # 6.77: the radius of the smallest u0 the code can form

GRID_QUADS = 2048 * 256      # sched_launch caps the grid at 2048 blocks of 256 lanes: quads past this are the loop's second trip

# The tail seeds: searched once by search_tail_seeds() below -- counter (0, 0, 0, 0) (quad 0, step 0, clip0 0), key (s, 0) for
# s = 0 .. 2^28 - 1 in chunks of 2^22.
#   TAIL_SEED_U0_ONE     the first s whose r0 >= 2^32 - 128: f32(r0) = 2^32, u0 rounds to 1, ra = sqrt(-0)
#   TAIL_SEED_U0_SMALL   of the s whose r0 < 2^12, the one with the smallest r0: the largest |z| of the range
# Both were found inside the 2^28 keys (the first after 16.4 million of them, at the expected rate of 3e-8 per key).
TAIL_SEED_U0_ONE, TAIL_R0_U0_ONE = 16390493, 4294967219           # r0 = 2^32 - 77
TAIL_SEED_U0_SMALL, TAIL_R0_U0_SMALL = 195960106, 13              # u0 = 13.5 * 2^-32, ra = 6.26


# ---------------------------------------------------------------------------------------------------------------------
# Philox4x32-10
# ---------------------------------------------------------------------------------------------------------------------
def philox4x32_10_scalar(counter, key):
    """Pure-Python integers: (c0, c1, c2, c3), (k0, k1) -> (r0, r1, r2, r3)."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def _u64(v):
    return np.asarray(v, dtype=np.uint64) & np.uint64(M32)


def philox4x32_10(counter, key):
    """Vectorised over numpy uint64 (32-bit values, masked after every step): counter = 4 and key = 2 arrays or integers that
    broadcast -> uint64 [..., 4]."""
    c0, c1, c2, c3 = (_u64(c) for c in counter)
    k0, k1 = (_u64(k) for k in key)
    m32, s32 = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2      # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & m32, p1 & m32, ((p0 >> s32) ^ c3 ^ k1) & m32, p0 & m32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m32, (k1 + np.uint64(PHILOX_W1)) & m32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


# ---------------------------------------------------------------------------------------------------------------------
# uniforms and normals
# ---------------------------------------------------------------------------------------------------------------------
def uniforms(r, defect=None):
    """r uint64 [..., 4] -> (u0, u1, u2, u3) float32, every operation in float32 as in philox_normal4."""
    f = np.asarray(r, dtype=np.uint64).astype(np.float32)      # round to nearest even, like the device conversion
    k, half, one = np.float32(2.0 ** -32), np.float32(0.5), np.float32(1.0)
    if defect == "half_offset_missing":
        half = np.float32(0.0)
    u0 = np.minimum((f[..., 0] + half) * k, one)
    u2 = np.minimum((f[..., 2] + half) * k, one)
    return u0, f[..., 1] * k, u2, f[..., 3] * k


def _normals(seed, quad, step, clip, defect=None):
    seed = int(seed)
    k1 = 0 if defect == "seed_hi_ignored" else seed >> 32
    r = philox4x32_10((quad, step, clip, 0), (seed & M32, k1))
    u0, u1, u2, u3 = (u.astype(np.float64) for u in uniforms(r, defect))
    with np.errstate(divide="ignore"):
        ra, rb = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    ra, rb = ra + 0.0, rb + 0.0                                  # sqrt(-0) = -0 -> +0
    a0, a1 = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    t0, t1 = (np.cos(a0), np.sin(a0)), (np.cos(a1), np.sin(a1))
    if defect == "sin_cos_swapped":
        t0, t1 = t0[::-1], t1[::-1]
    z = np.stack([ra * t0[0], ra * t0[1], rb * t1[0], rb * t1[1]], axis=-1)
    return z, np.stack([ra, ra, rb, rb], axis=-1)


def normals64(seed, quad, step, clip):
    """Box-Muller in fp64 on the fp32 uniforms of counter (quad, step, clip, 0), key (seed & 0xffffffff, seed >> 32):
    float64 [..., 4] = (ra cos 2 pi u1, ra sin 2 pi u1, rb cos 2 pi u3, rb sin 2 pi u3)."""
    return _normals(seed, quad, step, clip)[0]


DEFECTS = ("step_ignored", "t_for_k", "clip_ignored", "seed_hi_ignored", "quad_not_restarted", "quad_from_global_index",
           "sin_cos_swapped", "half_offset_missing")


def _model(seed, clip0, k, n, n_per_clip, defect=None, t=None):
    assert n % 4 == 0 and n_per_clip % 4 == 0 and (defect is None or defect in DEFECTS)
    e = np.arange(0, n, 4, dtype=np.int64)
    clip = e // n_per_clip
    if defect == "quad_not_restarted":                      # the counter runs on over the clip boundary
        quad = e >> 2
    elif defect == "quad_from_global_index":                # the lane's first-trip index instead of the loop variable
        quad = ((((e >> 2) % GRID_QUADS) << 2) - clip * n_per_clip) >> 2
    else:
        quad = (e - clip * n_per_clip) >> 2
    word = np.zeros_like(clip) if defect == "clip_ignored" else clip0 + clip
    step = 0 if defect == "step_ignored" else (int(t) if defect == "t_for_k" else int(k))
    z, ra = _normals(seed, quad & M32, step, word & M32, defect)
    return z.reshape(-1), ra.reshape(-1)


def noise_model(seed, clip0, k, n, n_per_clip, defect=None, t=None):
    """The z (float64 [n]) of a whole buffer at step k, as sched_noise4 keys it.  t (= tseq[k]) is read by defect 't_for_k' only."""
    return _model(seed, clip0, k, n, n_per_clip, defect, t)[0]


def noise_bound(z_ref, ra, e_trig=None):
    """The per-element tolerance of the module docstring."""
    e_trig = E_TRIG if e_trig is None else e_trig
    return ra * e_trig + np.abs(z_ref) * E_REL + NOISE_TINY


def noise_reference(seed, clip0, k, n, n_per_clip, e_trig=None):
    """-> (z_ref, ra, bound), float64 [n] each."""
    z, ra = _model(seed, clip0, k, n, n_per_clip)
    return z, ra, noise_bound(z, ra, e_trig)


def first_r0(seed, clip0=0):
    """r0 of quad 0, step 0 of a seed: what the tail seeds are chosen by."""
    return philox4x32_10_scalar((0, 0, clip0, 0), (seed & M32, seed >> 32))[0]


def search_tail_seeds(n_keys=1 << 28, chunk=1 << 22):
    """The search behind TAIL_SEED_*: -> ((seed, r0) of the first r0 >= 2^32 - 128 or of the largest r0 seen, found?,
    (seed, r0) of the smallest r0 seen).  A minute or two of numpy."""
    top, small = (None, -1), (None, 1 << 32)
    found = False
    for s0 in range(0, n_keys, chunk):
        s = np.arange(s0, min(s0 + chunk, n_keys), dtype=np.uint64)
        r0 = philox4x32_10((0, 0, 0, 0), (s, 0))[..., 0]
        if not found:
            hit = np.nonzero(r0 >= np.uint64((1 << 32) - 128))[0]
            if hit.size:
                top, found = (int(s[hit[0]]), int(r0[hit[0]])), True
            elif int(r0.max()) > top[1]:
                top = (int(s[r0.argmax()]), int(r0.max()))
        if int(r0.min()) < small[1]:
            small = (int(s[r0.argmin()]), int(r0.min()))
    return top, found, small


# ---------------------------------------------------------------------------------------------------------------------
# the update expressions: unfused, in the kernel's order, in the dtype of the operands (fp32: the twin of sched_update4 and of
# the CFG mix of sched_kernel; fp64: the reference the rounding bounds are counted against).  Coefficients are Python floats
# holding fp32 values.
# ---------------------------------------------------------------------------------------------------------------------
def _c(v, like):
    return torch.tensor(float(v), dtype=like.dtype)


def cfg_mix(x0, x0u, s):
    return x0u + _c(s, x0) * (x0 - x0u)


def update_mode0(c1, c2, sg, t, x0, x, z=None):
    o = _c(c1, x0) * x0 + _c(c2, x) * x
    if t > 0:
        o = o + _c(sg, x0) * z
    return o


def update_mode1(sra, srm1, san, cn, x0, x):
    eps = (_c(sra, x) * x - x0) / _c(srm1, x)
    return x0 * _c(san, x0) + _c(cn, x0) * eps


def update_mode3(a, b, c, s, x0, x, h=None, z=None):
    o = _c(b, x0) * x0 + _c(a, x) * x
    if c != 0.0:
        o = o + _c(c, x0) * h
    if s != 0.0:
        o = o + _c(s, x0) * z
    return o


def gamma(r):
    return r * U / (1.0 - r * U)


def mix_bound(x0, x0u, s):
    """|fp32 mix - fp64 mix|: 3 roundings over |u| + |s| (|x0| + |u|)."""
    x0, x0u = x0.double(), x0u.double()
    return gamma(3) * (x0u.abs() + abs(s) * (x0.abs() + x0u.abs()))


def mode0_bound(c1, c2, sg, t, x0, x, z=None, e_x0=None):
    a = abs(c1) * x0.double().abs() + abs(c2) * x.double().abs()
    r = 3
    if t > 0:
        a, r = a + abs(sg) * z.double().abs(), 5
    return gamma(r) * a + (abs(c1) * e_x0 * (1.0 + gamma(r)) if e_x0 is not None else 0.0)


def mode1_bound(sra, srm1, san, cn, x0, x, e_x0=None):
    x0a, xa = x0.double().abs(), x.double().abs()
    a = abs(san) * x0a + abs(cn / srm1) * (abs(sra) * xa + x0a)
    return gamma(6) * a + ((abs(san) + abs(cn / srm1)) * e_x0 * (1.0 + gamma(6)) if e_x0 is not None else 0.0)


def mode3_bound(a, b, c, s, x0, x, h=None, z=None, e_x0=None):
    t = abs(b) * x0.double().abs() + abs(a) * x.double().abs()
    r = 3
    if c != 0.0:
        t, r = t + abs(c) * h.double().abs(), r + 2
    if s != 0.0:
        t, r = t + abs(s) * z.double().abs(), r + 2
    return gamma(r) * t + (abs(b) * e_x0 * (1.0 + gamma(r)) if e_x0 is not None else 0.0)


def f32(v):
    """A Python float holding the fp32 rounding of v."""
    return float(np.float32(v))


def update_operands(n, seed=0):
    """Seeded fp32 operands of an update of n elements: x0, x0u, x, h (the history), z (stand-in noise for the host checks)."""
    g = torch.Generator().manual_seed(4200 + 17 * seed + n)
    return {name: torch.randn(n, generator=g) * sc + off for name, sc, off in
            (("x0", 1.0, 0.25), ("x0u", 1.0, -0.5), ("x", 2.0, 0.0), ("h", 1.0, 0.1), ("z", 1.0, 0.0))}


# coefficient sets (fp32 values) of the update checks: name -> arguments in the order of update_mode*
MODE0_COEFS = {"t5": (f32(0.731), f32(0.268), f32(0.0547), 5), "t0": (f32(0.999), f32(0.0013), f32(0.3), 0)}
MODE1_COEFS = {"mid": (f32(1.83), f32(1.53), f32(0.61), f32(0.79))}
MODE3_COEFS = {"all": (f32(0.83), f32(0.41), f32(-0.22), f32(0.37)), "no_hist": (f32(0.83), f32(0.41), 0.0, f32(0.37)),
               "no_noise": (f32(0.83), f32(0.41), f32(-0.22), 0.0), "plain": (f32(0.83), f32(0.41), 0.0, 0.0)}
CFG_SCALE = 2.5


# ---------------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------------
TSEQ = [7, 3, 0, 5, 1, 2, 9, 8, 6, 4]      # tseq[k] != k at every k the cases use; tseq[2] = 0: the launch that draws nothing
STEPS = [0, 1, 2, 9]
CLIP0S = [0, 5, 2 ** 31 - 4]
SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 0xDEADBEEF00000000, 2 ** 64 - 1]      # + the two tail seeds (tail_seeds())


def tail_seeds():
    return [TAIL_SEED_U0_ONE, TAIL_SEED_U0_SMALL]


class NoiseCase(namedtuple("NoiseCase", "seed clip0 k n n_per_clip")):
    @property
    def id(self):
        return f"seed{self.seed:#x}-clip{self.clip0}-k{self.k}-n{self.n}x{self.n_per_clip}"

    @property
    def t(self):
        return TSEQ[self.k]


def _noise_cases():
    cs = [NoiseCase(1, 0, k, 4, 4) for k in STEPS]                                           # one quad, every step
    cs += [NoiseCase(2 ** 32 + 1, c0, k, 24, 8) for c0 in CLIP0S for k in STEPS]             # three clips of two quads
    cs += [NoiseCase(s, 5, 1, 24, 8) for s in SEEDS + tail_seeds()]
    cs += [NoiseCase(s, 0, 0, 4, 4) for s in tail_seeds()]                                   # the tail quads themselves
    return list(dict.fromkeys(cs))


GRID_N = 2 ** 21 + 2 ** 12                 # 513 * 4096: the elements from 2^21 on are the second trip of the grid-stride loop


def grid_cases():
    return [NoiseCase(2 ** 32 + 1, 5, 1, GRID_N, 4096), NoiseCase(2 ** 32 + 1, 5, 1, GRID_N, GRID_N)]


def noise_cases():
    return _noise_cases()


# the slots of B: keys {seed, clip id}, state {k, t, live, run}; slot 1 is not live
SLOT_N_PER_CLIP = 8
SLOT_KEYS = [(2 ** 32 + 3, 1), (7, 2 ** 31 - 1), (0xDEADBEEF00000000, 0)]
SLOT_STATE = [(3, TSEQ[3], 1, 1), (6, TSEQ[6], 0, 1), (9, TSEQ[9], 1, 1)]

# defect -> (the case that targets it, the first element the defect can reach).  A defect of the counter's quad word leaves the
# first clip / the first trip of the loop as it is: its case counts the elements after them.
DefectCase = namedtuple("DefectCase", "case lo hi")


def defect_cases():
    three = NoiseCase(2 ** 32 + 1, 5, 1, 24, 8)
    return {
        "step_ignored": DefectCase(three, 0, 24),
        "t_for_k": DefectCase(three, 0, 24),
        "clip_ignored": DefectCase(three, 0, 24),
        "seed_hi_ignored": DefectCase(three, 0, 24),
        "quad_not_restarted": DefectCase(three, 8, 24),
        "quad_from_global_index": DefectCase(grid_cases()[0], 2 ** 21, GRID_N),
        "sin_cos_swapped": DefectCase(three, 0, 24),
        # (f32(r0) + 0.5f) is f32(r0) again from r0 = 2^24 on: only a small r0 shows the offset, and only in the pair that r0 feeds
        "half_offset_missing": DefectCase(NoiseCase(TAIL_SEED_U0_SMALL, 0, 0, 4, 4), 0, 2),
    }


def as_i64(v):
    """A 64-bit word as the int64 a torch tensor holds."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= 1 << 63 else v
