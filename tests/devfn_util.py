"""ctypes binding of libd2d_probe.so's d2d_probe_device_fn (include/d2d_hip_diag.h, csrc/d2d_devfn.hip: the device functions the
kernels share, one at a time behind wrapper kernels) and the references test_gpu_devfn.py holds them against: NumPy float64, exact
integer restatements, and the lane-exchange trees restated step by step in float32.  Nothing here is measured against the code
under test; test_devfn_cpu.py checks these references against independent ones."""
import ctypes as C
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LIB_PATH = ROOT / 'gym_d2d_amd' / 'lib' / 'libd2d_probe.so'
CSRC = ROOT / 'gym_d2d_amd' / 'csrc'

# enum d2d_devfn (include/d2d_hip_diag.h)
FN = {name: k for k, name in enumerate(('POW10_TENTH', 'POW_NEG_HALF', 'POW_K_GAINS', 'PAIR_GAIN', 'PRECISE_DIV', 'FAST_DIV', 'COS_TURNS',
                                        'PHILOX_STEP', 'PHILOX_NORMAL', 'WAVE_SUM', 'WAVE_SUM_HALVES', 'WAVE_MAX', 'WAVE_MIN', 'SORT8',
                                        'OBS_SRC_COL', 'SAME_RB'))}
FN_COUNT = 16
SENTINEL = 0x5A5A5A5A                                    # D2D_DEVFN_SENTINEL
PL_INV_SQUARE, PL_POWER, PL_POWK = 0, 1, 4               # PlMode (csrc/d2d_internal.h)
LIST_EMPTY = 0xFFFF                                      # d2d_step_device.h
KEY_SHIFT, MAX_LINKS, MAX_RBS = 11, 2048, 8192           # d2d_same_rb.h
# every name the wrappers call and none of which csrc/d2d_devfn.hip may define
TESTED = ('pow10_tenth', 'pow_neg_half', 'pow_k_gains', 'pair_gain', 'precise_div', 'fast_div', 'cos_turns', 'philox_step', 'philox_normal',
          'wave_sum', 'wave_sum_halves', 'wave_reduce', 'dpp_key', 'dpp_f32', 'sort8', 'obs_src_col', 'same_rb_keys', 'same_rb_rank',
          'same_rb_starts')
_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(f'{LIB_PATH} is missing - build it with `python -m gym_d2d_amd.build`')
        lib = C.CDLL(str(LIB_PATH))
        lib.d2d_probe_last_error.restype = C.c_char_p
        lib.d2d_probe_device_fn.restype = C.c_int
        lib.d2d_probe_device_fn.argtypes = [C.c_int32] + [C.c_void_p] * 5 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
        _lib = lib
    return _lib


def device_fn(fn, a=0, b=0, c=0, out0=0, out1=0, n=0, k0=0, k1=0, stream=0):
    """d2d_probe_device_fn: `fn` a name of FN or an id; the pointers are plain ints (0 = null).  ValueError with the library's text."""
    fn = FN[fn] if isinstance(fn, str) else int(fn)
    lib = load()
    rc = lib.d2d_probe_device_fn(fn, *(C.c_void_p(int(p) or None) for p in (a, b, c, out0, out1)), int(n), int(k0), int(k1),
                                 C.c_void_p(int(stream) or None))
    if rc:
        raise ValueError(lib.d2d_probe_last_error().decode(errors='replace'))


# ------------------------------------------------------------------------------------------------ float32 helpers
F32_MIN_NORMAL = float(np.float32(2.0 ** -126))
F32_MAX = float(np.finfo(np.float32).max)


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def ulp_distance(a, b):
    """Distance in float32 steps between two arrays of finite float32 of the same sign."""
    return np.abs(f32_bits(a).astype(np.int64) - f32_bits(b).astype(np.int64))


def neighbours(x):
    """x with its float32 predecessor and successor, flattened."""
    x = np.asarray(x, dtype=np.float32)
    return np.concatenate([np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))])


def rel_err(got, ref):
    """|got - ref| / |ref| in float64 (ref != 0)."""
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.abs(ref)


def worst(err, *where):
    """(max of err, the values of `where` at it) - what a test prints before it asserts."""
    k = int(np.nanargmax(err))
    return float(err[k]), tuple(np.asarray(w).ravel()[k].item() for w in where)


# ------------------------------------------------------------------------------------------------ the power laws
def head_tail(e):
    """(head, tail) of -e / 2 for a float64 exponent e, as the host builds the pair (d2d_capi.hip::refresh_tables: `hd = -0.5 * expo`,
    `head = (float)hd` with `hb &= 0xFFFFF000u`, `tail = (float)(hd - (double)head)`): the head is float32(-e/2) with its low 12
    mantissa bits cleared, the tail float32 of what is left in double."""
    hd = -0.5 * np.asarray(e, dtype=np.float64)
    head = (hd.astype(np.float32).view(np.uint32) & np.uint32(0xFFFFF000)).view(np.float32)
    tail = (hd - head.astype(np.float64)).astype(np.float32)
    return head, tail


E_FIXED = np.array([2.0, 2.5, 3.0, 3.5, 3.76, 4.0, 4.4, 4.6])     # 2.5, 3.0, 3.5: head * exponent a half-integer, rintf's tie


WIDE = slice(8, 8 + (1 << 20))                      # the drawn (e, d2) pairs inside _pow_neg_half_inputs()


def pow_neg_half_inputs():
    """(d2, e) of the pow_neg_half tests: the fixed exponents and 2^20 drawn ones, each under one log-uniform d2 in [1e-2, 1e12]; then
    every edge argument (2^j for j in [-6, 40] with its float32 neighbours, two sweeps of 4096 mantissas across [2^16, 2^17)) under
    every fixed exponent and 56 of the drawn ones."""
    rng = np.random.default_rng(20240611)
    e = np.concatenate([E_FIXED, rng.uniform(2.0, 4.6, size=1 << 20)])
    d2_wide = (10.0 ** rng.uniform(-2, 12, size=len(e))).astype(np.float32)                    # log-uniform in [1e-2, 1e12]
    pow2 = neighbours(np.float32(2.0) ** np.arange(-6, 41, dtype=np.float32))              # 2^j and its float32 neighbours
    binade = (65536.0 * (1.0 + np.arange(4096) / 4096.0)).astype(np.float32)                  # 4096 mantissas across [2^16, 2^17)
    fine = np.nextafter(np.float32(65536.0), np.float32(np.inf)) + np.arange(0, 4096 * 1999, 1999).astype(np.float32) / np.float32(128.0)
    edge = np.concatenate([pow2, binade, fine.astype(np.float32)])
    e_edge = np.concatenate([E_FIXED, e[8:64]])
    d2 = np.concatenate([d2_wide, np.tile(edge, len(e_edge))])
    ee = np.concatenate([e, np.repeat(e_edge, len(edge))])
    return d2, ee


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; one rounding to float64, one to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_pow10_tenth(p):
    """pow10_tenth's arithmetic as d2d_step_device.h writes it, in NumPy float32, with exp2 correctly rounded (float64, rounded once):
    the algorithm's own error, without the hardware's v_exp_f32."""
    fp = np.asarray(p).astype(np.float32)
    xh = fp * np.float32(0.3321533203125)
    ip = np.floor(xh)
    fr = _fma32(fp, np.full_like(fp, np.float32(3.948917623623e-05)), xh - ip)
    with np.errstate(over='ignore'):
        return np.ldexp(np.exp2(fr.astype(np.float64)).astype(np.float32).astype(np.float64), ip.astype(np.int64)).astype(np.float32)


def emulate_pow_neg_half(d2, head, tail):
    """pow_neg_half's arithmetic as written (contraction off), in NumPy float32 with log2 / exp2 correctly rounded."""
    d2 = np.asarray(d2, dtype=np.float32)
    m, ex = np.frexp(d2)
    fe = ex.astype(np.float32)
    l = np.log2(m.astype(np.float64)).astype(np.float32)
    p = head * fe
    ip = np.rint(p)
    t = tail * (l + fe)
    fr = (p - ip) + _fma32(head, l, t)
    with np.errstate(over='ignore'):
        return np.ldexp(np.exp2(fr.astype(np.float64)).astype(np.float32).astype(np.float64), ip.astype(np.int64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the lane exchange
_LANE = np.arange(64)
_ROW = _LANE >> 4


def wave_sum_tree(v, levels=6):
    """wave_sum's tree (d2d_step_device.h) restated in float32, step by step in the header's order, on [..., 64]: quad xor 1, quad xor
    2, half-row mirror, row mirror, row broadcast 15 into rows 1 and 3, row broadcast 31 into rows 2 and 3.  A lane the row mask
    leaves out adds the `old` operand, +0.0.  Returns all 64 lanes after `levels` steps: lane 63 holds the wave's sum after six,
    lanes 31 and 63 the halves' after five."""
    v = np.array(v, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        v = v + v[..., _LANE ^ 1]
        v = v + v[..., _LANE ^ 2]
        v = v + v[..., (_LANE & ~7) | (7 - (_LANE & 7))]
        v = v + v[..., (_LANE & ~15) | (15 - (_LANE & 15))]
        if levels >= 5:
            src = v[..., np.maximum(_ROW * 16 - 1, 0)]                    # lane 15 of the row before
            v = v + np.where((_ROW == 1) | (_ROW == 3), src, np.float32(0.0))
        if levels >= 6:
            v = v + np.where(_ROW >= 2, v[..., 31:32], np.float32(0.0))
    return v


def wave_sum_ref(v):
    return wave_sum_tree(v)[..., 63]


def wave_sum_halves_ref(v):
    t = wave_sum_tree(v, levels=5)
    return t[..., 31], t[..., 63]


def wave_sum_cases(rng):
    """[cases, 64] float32 where the association of the additions matters, and where a wrong row mask or control shows."""
    cases = [np.eye(64, dtype=np.float32)]                                                     # one-hot: a 1.0 in each lane in turn
    mixed = (10.0 ** rng.uniform(-8, 8, size=(64, 64))).astype(np.float32)                     # 1e-8 .. 1e8 in one wave
    cases += [mixed, mixed * np.where(np.arange(64) & 1, -1, 1).astype(np.float32)]            # ... and with alternating signs
    cases.append(rng.standard_normal((64, 64)).astype(np.float32))
    cases.append((np.arange(64, dtype=np.float32) + 1.0)[None, :] * np.float32(1.0000001) ** np.arange(8, dtype=np.float32)[:, None])
    inf = rng.standard_normal((8, 64)).astype(np.float32)
    for r in range(4):
        inf[2 * r, 16 * r + int(rng.integers(16))] = np.inf                                   # an inf in one row ...
        inf[2 * r + 1, np.arange(4) * 16 + rng.integers(16, size=4)] = -np.inf                # ... and one in each row
    cases.append(inf)
    nan = rng.standard_normal((64, 64)).astype(np.float32)
    nan[np.arange(64), np.arange(64)] = np.nan                                                 # a NaN in one lane, each in turn
    cases.append(nan)
    return np.concatenate(cases, axis=0)


def wave_key_cases(rng, largest):
    """[cases, 64] uint64 keys for wave_reduce<largest>."""
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    ext, rest = (full, np.uint64(0)) if largest else (np.uint64(0), full)
    hot = np.full((64, 64), rest, dtype=np.uint64)
    hot[np.arange(64), np.arange(64)] = ext                                                    # each lane in turn holds the extreme
    hot2 = rng.integers(1 << 20, 1 << 40, size=(64, 64)).astype(np.uint64)
    hot2[np.arange(64), np.arange(64)] = np.uint64(1 << 50) if largest else np.uint64(5)      # ... among random others
    equal = np.repeat(rng.integers(0, 1 << 63, size=(8, 1)).astype(np.uint64), 64, axis=1)
    low = (np.uint64(0x1234567) << np.uint64(32)) | rng.integers(0, 1 << 32, size=(16, 64)).astype(np.uint64)          # low word only
    high = (rng.integers(0, 1 << 32, size=(16, 64)).astype(np.uint64) << np.uint64(32)) | np.uint64(0x89ABCDEF)         # high word only
    hi = rng.permuted(np.tile(np.arange(64, dtype=np.uint64), (16, 1)), axis=1)
    opposite = (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - hi * np.uint64(0x01010101))   # high words order against low words
    ends = rng.integers(0, 1 << 63, size=(16, 64)).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    ends[np.arange(16), rng.integers(64, size=16)] = np.uint64(0)
    ends[np.arange(16), (rng.integers(63, size=16) + 1 + np.argmin(ends, axis=1)) % 64] = full                           # 0 and all-ones present
    rand = rng.integers(0, 1 << 63, size=(64, 64)).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(64, 64)).astype(np.uint64)
    return np.concatenate([hot, hot2, equal, low, high, opposite, ends, rand], axis=0)


# ------------------------------------------------------------------------------------------------ integer functions
def obs_src_col_ref(f, i):
    """The source float inside T_flat of output column f of row i, from the ordering obs_fn.py:43-53 states (own link first, then
    the others in agent order): slot k = f // 6 shows link i (k = 0), k - 1 (1 <= k <= i) or k (k > i)."""
    f, i = np.asarray(f, dtype=np.int64), np.asarray(i, dtype=np.int64)
    k = f // 6
    link = np.where(k == 0, i, np.where(k <= i, k - 1, k))
    return 6 * link + f % 6


def same_rb_ref(rb_row, R):
    """(slot[N], start[R + 1]) of one env: slot = the position in np.lexsort((j, rb')), rb' = rb or R where rb is outside [0, R);
    start[r] = the first sorted entry whose rb' is >= r."""
    rb_row = np.asarray(rb_row, dtype=np.int64)
    n = len(rb_row)
    eff = np.where((rb_row >= 0) & (rb_row < R), rb_row, R)
    order = np.lexsort((np.arange(n), eff))
    slot = np.empty(n, dtype=np.int64)
    slot[order] = np.arange(n)
    return slot, np.searchsorted(eff[order], np.arange(R + 1), side='left')


def same_rb_rows(rng, N, R):
    """The four envs of one (N, R) shape: random in [-2, R + 2), all on one RB, all out of range (INT_MIN and INT_MAX among them), one
    link per RB with empty RBs between (R > N; else the links dealt round the RBs)."""
    rows = np.empty((4, N), dtype=np.int32)
    rows[0] = rng.integers(-2, R + 2, size=N)
    rows[1] = int(rng.integers(R))
    rows[2] = rng.choice(np.array([-1, -2, R, R + 1, -2 ** 31, 2 ** 31 - 1, 2 ** 30, -2 ** 30], dtype=np.int64), size=N)
    rows[2, 0], rows[2, -1] = -2 ** 31, 2 ** 31 - 1
    if N == 1:
        rows[2, 0] = -2 ** 31
    rows[3] = rng.permutation((np.arange(N) * (R // N)) if R > N else (np.arange(N) % R))
    return rows


def philox_patterns(rng, n, words):
    """[n, words] uint32: all-zero, all-ones, every single-bit pattern of the words, then random."""
    out = rng.integers(0, 1 << 32, size=(n, words), dtype=np.uint64).astype(np.uint32)
    out[0], out[1] = 0, 0xFFFFFFFF
    bits = min(32 * words, n - 2)
    out[2:2 + bits] = 0
    out[2 + np.arange(bits), np.arange(bits) // 32] = np.uint32(1) << (np.arange(bits) % 32).astype(np.uint32)
    return out
