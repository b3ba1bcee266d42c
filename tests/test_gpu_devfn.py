"""The device functions the kernels share (csrc/d2d_step_device.h, d2d_wave_key.h, d2d_same_rb.h), each by direct launch through
libd2d_probe.so's wrapper kernels (csrc/d2d_devfn.hip, tests/devfn_util.py) against a reference of its own: NumPy float64 for the
arithmetic, exact integer restatements, and the lane-exchange tree restated step by step in float32.  The bound a test asserts is the
figure the function's header comment states, mirrored below next to the line that states it; every test prints the worst error it
saw and where, before it asserts.  Every output sits between guard bands that are checked."""
import numpy as np
import pytest
import torch

import devfn_util as dv
from guard_util import Guarded
from oracle import d2d_oracle as orc

pytestmark = pytest.mark.gpu

# the figures the headers state (csrc/d2d_step_device.h)
POW_NEG_HALF_REL = 2.7e-7        # "(d^2)^h for h = -e/2 given as a head + tail pair ... to 2.7e-7 relative" (corrected from ~2.5e-7)
POW10_TENTH_REL = 1.5e-7         # "10^(p/10) for an integer power level p (dBm -> mW), ~1.5e-7 relative"
POW_K_REL = 6.9e-7               # pow_k_gains: "6.9e-7 relative in all" (corrected from about 4e-7)
FAST_DIV_REL = 2.0e-7            # fast_div: "x / y with v_rcp_f32 (1 ulp) ...: 2e-7 relative"
PRECISE_DIV_ULP = 1              # precise_div: "x / y to within an ulp"
PHILOX_NORMAL_ABS = 5.6e-7       # philox_normal: "Box-Muller to 5.6e-7 absolute in z" (corrected from ~1e-7)
COS_TURNS_ABS = 1.07e-7          # cos_turns: "1.07e-7 absolute at worst over all 2^24 arguments" (measured here; twice it is asserted)
COS_TURNS_CAP = 2.0 ** -22       # ... and never asserted wider than this

_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32,
          np.dtype(np.uint64): torch.int64, np.dtype(np.int64): torch.int64}


def _dev(x):
    """A host array on the device, its bytes unchanged (unsigned types travel as the signed type of their width)."""
    x = np.ascontiguousarray(x)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(x.dtype)
    return torch.from_numpy(x.view(signed) if signed else x).cuda()


def call(fn, ins, outs, n, k0=0, k1=0):
    """One launch of `fn`: ins = host arrays (a, b, c), outs = [(shape, numpy dtype)] for out0, out1, each in a guarded
    allocation filled with its byte pattern.  Returns the outputs as host arrays; asserts the guard bands."""
    dev = [_dev(x) for x in ins]
    g = [Guarded(shape, _TORCH[np.dtype(dt)]) for shape, dt in outs]
    ptrs = [t.data_ptr() for t in dev] + [0] * (3 - len(dev))
    optrs = [x.array.data_ptr() for x in g] + [0] * (2 - len(g))
    dv.device_fn(fn, *ptrs, *optrs, n=n, k0=k0, k1=k1, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(x.intact() for x in g), f'{fn}: a store outside the output'
    return [x.array.cpu().numpy().view(np.dtype(dt)) for x, (shape, dt) in zip(g, outs)]


def f32(fn, *ins, k0=0, k1=0):
    n = len(ins[0])
    return call(fn, ins, [((n,), np.float32)], n, k0, k1)[0]


# ------------------------------------------------------------------------------------------------ powers and divisions
def test_pow10_tenth_every_level():
    """pow10_tenth(p) for every integer p in [-4095, 4095] against 10.0 ** (p / 10) in float64: relative error where the reference
    is a normal float32 (p in [-379, 385]), +inf above, finite and below the smallest normal beneath, non-decreasing throughout.
    MI355X: worst 7.14e-8 at p = -219 (stated ~1.5e-7)."""
    p = np.arange(-4095, 4096, dtype=np.int32)
    got = f32('POW10_TENTH', p)
    with np.errstate(over='ignore'):
        ref = 10.0 ** (p.astype(np.float64) / 10.0)                                            # +inf from p = 3083 on
    normal = (ref >= dv.F32_MIN_NORMAL) & (ref <= dv.F32_MAX)
    assert p[normal].min() == -379 and p[normal].max() == 385
    rel = np.zeros(len(p))
    rel[normal] = dv.rel_err(got[normal], ref[normal])
    err, at = dv.worst(rel, p)
    print(f'pow10_tenth: worst relative error {err:.3e} at p = {at[0]} (stated {POW10_TENTH_REL:.1e})')
    assert np.all(np.isposinf(got[p >= 386]))
    low = got[p <= -380]
    assert np.all(np.isfinite(low)) and np.all(low >= 0.0) and np.all(low < 2.0 ** -126 * (1.0 + POW10_TENTH_REL))
    assert np.all(np.diff(got.astype(np.float64)[np.isfinite(got)]) >= 0.0) and np.all(np.isfinite(got[p < 386]))
    assert err <= POW10_TENTH_REL


E_FIXED, WIDE, _pow_neg_half_inputs = dv.E_FIXED, dv.WIDE, dv.pow_neg_half_inputs


def test_pow_neg_half_against_float64():
    """pow_neg_half(d2, (head, tail)) against np.power(float64(d2), -e / 2): e in {2, 2.5, 3, 3.5, 3.76, 4, 4.4, 4.6} and 2^20 draws
    in [2, 4.6]; d2 log-uniform in [1e-2, 1e12], every 2^j (j in [-6, 40]) with its float32 neighbours, 4096 mantissas across one
    binade.  MI355X: worst 2.67e-7 at d2 = 4815247360, e = 4.2888 (the header stated ~2.5e-7 and now states 2.7e-7)."""
    d2, e = _pow_neg_half_inputs()
    head, tail = dv.head_tail(e)
    ref = np.power(d2.astype(np.float64), -0.5 * e)
    # a normal float32 on this domain: (1e12)^-2.3 = 2.6e-28 among the drawn pairs (2.0e-28 at the successor of 2^40) .. (1e-2)^-2.3 = 3.9e4
    assert 2.0e-28 <= ref.min() and ref[WIDE].min() >= 2.5e-28 and ref.max() <= 3.99e4 and ref.min() >= dv.F32_MIN_NORMAL
    got = f32('POW_NEG_HALF', d2, head, tail)
    err, at = dv.worst(dv.rel_err(got, ref), d2, e)
    print(f'pow_neg_half: worst relative error {err:.3e} at d2 = {at[0]!r}, e = {at[1]!r} (stated {POW_NEG_HALF_REL:.1e})')
    err_w, at_w = dv.worst(dv.rel_err(got[WIDE], ref[WIDE]), d2[WIDE], e[WIDE])
    print(f'pow_neg_half: worst on the drawn pairs alone {err_w:.3e} at d2 = {at_w[0]!r}, e = {at_w[1]!r}')
    assert np.all(np.isfinite(got)) and err <= POW_NEG_HALF_REL


def test_pow_neg_half_specials():
    """d2 == 0 gives +inf (what the header's clamp of log2(0) is for), +inf gives 0, NaN gives NaN, a subnormal d2 no NaN - under every
    exponent of the fixed set."""
    head, tail = dv.head_tail(E_FIXED)
    for d2, check in ((0.0, np.isposinf), (np.inf, lambda g: g == 0.0), (np.nan, np.isnan), (1.0e-40, lambda g: ~np.isnan(g)),
                      (float(np.float32(2.0 ** -149)), lambda g: ~np.isnan(g))):
        got = f32('POW_NEG_HALF', np.full(len(E_FIXED), d2, dtype=np.float32), head, tail)
        assert np.all(check(got)), (d2, got)
        same = f32('PAIR_GAIN', np.full(len(E_FIXED), d2, dtype=np.float32), head, tail, k0=dv.PL_POWER)
        assert np.array_equal(dv.f32_bits(same), dv.f32_bits(got)) or np.all(np.isnan(got))


def _pow_k_inputs(n=1 << 17):
    rng = np.random.default_rng(77)
    phi = rng.uniform(-0.25, 0.25, size=n).astype(np.float32)
    phi[:3] = (0.0, 0.25, -0.25)
    phi[3:4099:3] = np.float32(0.0)
    d2 = (10.0 ** rng.uniform(-2, 6, size=n)).astype(np.float32)
    d2[:3] = (1.0e6, 1.0e6, 1.0e-2)
    edge = dv.neighbours(np.float32(2.0) ** np.arange(-6, 20, dtype=np.float32))
    d2[4099:4099 + len(edge)] = edge
    d2[4099 + len(edge):4099 + 2 * len(edge)] = edge
    phi[4099 + len(edge):4099 + 2 * len(edge)] = np.float32(0.25)
    return d2[:n - 3], phi[:n - 3]                        # a length that is no multiple of four: the NP = 4 form's last thread is partial


def test_pow_k_gains_against_float64_and_the_promised_bit_equalities():
    """pow_k_gains for k in 1..8, phi in [-1/4, 1/4] (0 and +-1/4 among them), d2 in [1e-2, 1e6] against
    d2 ** (-k / 2 + float64(phi)); and the equalities the header promises, as uint32 words: NP = 1 against NP = 4, KC = 4 against
    run-time k = 4, pair_gain<PL_POWK> against pow_k_gains<1>.  MI355X: worst 6.85e-7 at k = 6, d2 = 375800.44,
    phi = 0.2488; 5.56e-7 at k = 1 (the header stated about 4e-7 and now states 6.9e-7)."""
    d2, phi = _pow_k_inputs()
    zero = np.zeros_like(d2)
    worst_all = (0.0, None)
    for k in range(1, 9):
        got = f32('POW_K_GAINS', d2, phi, k0=k, k1=0)
        ref = np.power(d2.astype(np.float64), -0.5 * k + phi.astype(np.float64))
        assert ref.min() >= dv.F32_MIN_NORMAL and ref.max() <= dv.F32_MAX
        err, at = dv.worst(dv.rel_err(got, ref), d2, phi)
        print(f'pow_k_gains k = {k}: worst relative error {err:.3e} at d2 = {at[0]!r}, phi = {at[1]!r} (stated {POW_K_REL:.1e})')
        worst_all = max(worst_all, (err, (k,) + at), key=lambda t: t[0])
        four = f32('POW_K_GAINS', d2, phi, k0=k, k1=1)
        assert np.array_equal(dv.f32_bits(four), dv.f32_bits(got)), f'NP = 4 differs from NP = 1 at k = {k}'
        pair = f32('PAIR_GAIN', d2, phi, zero, k0=dv.PL_POWK, k1=k)
        assert np.array_equal(dv.f32_bits(pair), dv.f32_bits(got)), f'pair_gain<PL_POWK> differs from pow_k_gains<1> at k = {k}'
        if k == 4:
            fixed = f32('POW_K_GAINS', d2, phi, k0=4, k1=2)
            assert np.array_equal(dv.f32_bits(fixed), dv.f32_bits(got)), 'KC = 4 differs from run-time k = 4'
        for form in (0, 1):
            z = f32('POW_K_GAINS', np.zeros(5, dtype=np.float32), phi[:5], k0=k, k1=form)
            assert not np.any(np.isfinite(z)), (k, form, z)                                   # a zero distance ends non-finite
    print(f'pow_k_gains: worst relative error {worst_all[0]:.3e} at (k, d2, phi) = {worst_all[1]}')
    assert worst_all[0] <= POW_K_REL


def test_pair_gain_modes_are_the_functions_they_name():
    """pair_gain<PL_INV_SQUARE> is v_rcp_f32's value (the same word as 1.0f * v_rcp, which fast_div(1, d2) returns, and within an ulp
    of 1 / d2); pair_gain<PL_POWER> is pow_neg_half's word."""
    d2, e = _pow_neg_half_inputs()
    d2, e = d2[:1 << 16], e[:1 << 16]
    head, tail = dv.head_tail(e)
    inv = f32('PAIR_GAIN', d2, head, tail, k0=dv.PL_INV_SQUARE)
    rcp = f32('FAST_DIV', np.ones_like(d2), d2)
    assert np.array_equal(dv.f32_bits(inv), dv.f32_bits(rcp))
    assert dv.ulp_distance(inv, (1.0 / d2.astype(np.float64)).astype(np.float32)).max() <= 1
    power = f32('PAIR_GAIN', d2, head, tail, k0=dv.PL_POWER)
    assert np.array_equal(dv.f32_bits(power), dv.f32_bits(f32('POW_NEG_HALF', d2, head, tail)))


def _div_inputs():
    rng = np.random.default_rng(5)
    n = 1 << 20
    x = (10.0 ** rng.uniform(-30, 10, size=n)).astype(np.float32)
    y = (10.0 ** rng.uniform(-30, 10, size=n)).astype(np.float32)
    edge = dv.neighbours(np.float32(2.0) ** np.arange(-99, 34, dtype=np.float32))            # powers of two in [1e-30, 1e10], neighbours
    y[:len(edge) * 64] = np.tile(edge, 64)
    q = x.astype(np.float64) / y.astype(np.float64)
    keep = (q >= dv.F32_MIN_NORMAL) & (q <= dv.F32_MAX) & (y >= np.float32(1e-30)) & (y <= np.float32(1e10))
    return x[keep], y[keep], q[keep]


def test_precise_div_within_an_ulp():
    """precise_div(x, y), x and y log-uniform in [1e-30, 1e10] (y also the powers of two and their float32 neighbours), quotients
    that are normal float32: within 1 ulp of the float64 quotient rounded to float32.  MI355X: the same word as the rounded quotient in all
    1046473 cases (0 ulp), 5.96e-8 relative at worst."""
    x, y, q = _div_inputs()
    got = f32('PRECISE_DIV', x, y)
    ulps = dv.ulp_distance(got, q.astype(np.float32))
    err, at = dv.worst(dv.rel_err(got, q), x, y)
    print(f'precise_div: worst {int(ulps.max())} ulp from the rounded float64 quotient ({int((ulps > 0).sum())} of {len(q)} differ), '
          f'worst relative error {err:.3e} at x = {at[0]!r}, y = {at[1]!r}')
    assert np.all(np.isfinite(got)) and ulps.max() <= PRECISE_DIV_ULP


def test_fast_div_within_its_stated_figure():
    """fast_div(x, y) on the same arguments: within the header's 2e-7 relative of the float64 quotient.  MI355X: worst 1.45e-7 at
    x = 7.43e-3, y = 2.60e-17."""
    x, y, q = _div_inputs()
    got = f32('FAST_DIV', x, y)
    err, at = dv.worst(dv.rel_err(got, q), x, y)
    print(f'fast_div: worst relative error {err:.3e} at x = {at[0]!r}, y = {at[1]!r} (stated {FAST_DIV_REL:.1e})')
    assert err <= FAST_DIV_REL


# ------------------------------------------------------------------------------------------------ random numbers
def test_cos_turns_all_arguments():
    """cos_turns(u) for all 2^24 arguments u = k 2^-24 in one launch, against cos(2 pi k / 2^24) in float64: exact at the quarter
    turns, absolute error elsewhere.  Asserted at twice the worst measured on the MI355X (another clock or scheduling of the same
    instructions), never wider than 2^-22.  MI355X: worst 1.067e-7 at k = 2094735."""
    k = np.arange(1 << 24, dtype=np.int64)
    got = f32('COS_TURNS', (k.astype(np.float64) * 2.0 ** -24).astype(np.float32))
    quarter = 1 << 22
    assert [float(got[j * quarter]) for j in range(4)] == [1.0, 0.0, -1.0, 0.0]
    err = np.abs(got.astype(np.float64) - np.cos(k.astype(np.float64) * (2.0 * np.pi / (1 << 24))))
    w, at = dv.worst(err, k)
    print(f'cos_turns: worst absolute error {w:.3e} at k = {at[0]} of 2^24 (header: {COS_TURNS_ABS:.1e})')
    assert np.all(np.abs(got) <= 1.0)
    assert 0.0 < COS_TURNS_ABS and 2.0 * COS_TURNS_ABS <= COS_TURNS_CAP and w <= 2.0 * COS_TURNS_ABS


def test_philox_step_words():
    """philox_step's two output words for 2^16 (counter, key) pairs equal oracle.d2d_oracle.philox4x32_10 word for word: 128 keys
    (all-zero, all-ones, every single-bit pattern, random) by 512 counters each (the same patterns over four words, random)."""
    rng = np.random.default_rng(3)
    keys = dv.philox_patterns(rng, 128, 2)
    ctr = np.stack([dv.philox_patterns(rng, 512, 4) for _ in range(128)])                      # [128, 512, 4]
    key = np.repeat(keys[:, None, :], 512, axis=1)
    n = 128 * 512
    o0, o1 = call('PHILOX_STEP', [ctr.reshape(n, 4), key.reshape(n, 2)], [((n,), np.uint32), ((n,), np.uint32)], n)
    for g in range(128):
        w = orc.philox4x32_10(ctr[g, :, 0], ctr[g, :, 1], ctr[g, :, 2], ctr[g, :, 3], int(keys[g, 0]), int(keys[g, 1]))
        assert np.array_equal(o0[g * 512:(g + 1) * 512], w[0]) and np.array_equal(o1[g * 512:(g + 1) * 512], w[1]), g


SEED, STEP = 0x9E3779B97F4A7C15, 12345


def _normal_case(env, j, i, kind):
    spec = orc.ShadowSpec(seed=SEED, step=STEP)
    ref = spec.normals(env, j, i, kind)
    n = len(ref)
    ctr = np.stack([np.asarray(env, dtype=np.uint32), np.full(n, STEP, dtype=np.uint32),
                    (np.asarray(j, dtype=np.uint64) | (np.asarray(i, dtype=np.uint64) << np.uint64(16))).astype(np.uint32),
                    np.asarray(kind, dtype=np.uint32)], axis=1)
    key = np.tile(np.array([SEED & 0xFFFFFFFF, SEED >> 32], dtype=np.uint32), (n, 1))
    return f32('PHILOX_NORMAL', ctr, key), ref


def test_philox_normal_against_the_oracle_transform():
    """philox_normal on 2^20 counters against ShadowSpec.normals (the same words, Box-Muller in float64): absolute error in z.
    MI355X: worst 5.51e-7 at z = -2.88 (max |z| 5.12; the header stated ~1e-7 and now states 5.6e-7)."""
    rng = np.random.default_rng(11)
    n = 1 << 20
    env, j, i = np.arange(n, dtype=np.uint64), rng.integers(0, 1 << 16, size=n), rng.integers(0, 1 << 16, size=n)
    got, ref = _normal_case(env, j, i, rng.integers(0, 2, size=n))
    err, at = dv.worst(np.abs(got.astype(np.float64) - ref), ref)
    print(f'philox_normal: worst absolute error {err:.3e} at z = {at[0]!r}, max |z| = {np.abs(ref).max():.3f} (stated {PHILOX_NORMAL_ABS:.1e})')
    assert np.all(np.isfinite(got)) and err <= PHILOX_NORMAL_ABS


def test_philox_normal_at_the_ends_and_the_switch_of_the_logarithm():
    """Counters searched on the CPU with the oracle's generator until the radius word k1 = w0 >> 8 has fallen at least 8 times in
    each of: below 16, within 16 below 2^23, within 16 above 2^23, above 2^24 - 16 - the two ends of u1 and the switch between
    the logf and log1pf halves.  4 draws per 2^22 counters are expected in each; with this seed 2^23 counters hold 19, 12, 11 and 14.
    MI355X: worst absolute error in z 3.91e-7 (k1 < 16, z = 4.96), 1.04e-7, 5.7e-8 and 8.0e-11 (k1 > 2^24 - 16, z = -0.0012)."""
    chunk, found = 1 << 22, [[], [], [], []]
    for c in range(16):
        env = np.arange(c * chunk, (c + 1) * chunk, dtype=np.uint64)
        k1 = orc.philox4x32_10(env, np.uint64(STEP), np.uint64(7 | 9 << 16), np.uint64(0), SEED & 0xFFFFFFFF, SEED >> 32)[0] >> np.uint32(8)
        for r, m in enumerate((k1 < 16, (k1 >= (1 << 23) - 16) & (k1 < 1 << 23), (k1 >= 1 << 23) & (k1 < (1 << 23) + 16), k1 > (1 << 24) - 16)):
            found[r] += list(env[m])
        if min(len(f) for f in found) >= 8:
            break
    assert min(len(f) for f in found) >= 8, [len(f) for f in found]                          # the search found them
    names = ('k1 < 16', 'below 2^23', 'above 2^23', 'k1 > 2^24 - 16')
    worst_all = 0.0
    for name, envs in zip(names, found):
        envs = np.array(envs, dtype=np.uint64)
        got, ref = _normal_case(envs, np.full(len(envs), 7), np.full(len(envs), 9), np.zeros(len(envs), dtype=np.int64))
        err, at = dv.worst(np.abs(got.astype(np.float64) - ref), ref)
        print(f'philox_normal, {name}: {len(envs)} counters, worst absolute error {err:.3e} at z = {at[0]!r} (stated {PHILOX_NORMAL_ABS:.1e})')
        worst_all = max(worst_all, err)
    assert worst_all <= PHILOX_NORMAL_ABS


# ------------------------------------------------------------------------------------------------ lane exchange, exact
def _same_word_per_wave(out):
    return np.all(out.reshape(-1, 64) == out.reshape(-1, 64)[:, :1])


def _equal_words(got, ref):
    """Bit for bit; where the reference is NaN the payload is the adder's own business (an x86 host and the GPU propagate different
    ones), so there the result only has to be NaN."""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(dv.f32_bits(got)[~nan], dv.f32_bits(ref)[~nan])


@pytest.mark.parametrize('block', [64, 256])
def test_wave_sum_and_halves_bit_for_bit(block):
    """wave_sum and wave_sum_halves in workgroups of 64 and 256 threads: every lane of a wave holds the same word, and the word is
    the header's tree restated in float32 (devfn_util.wave_sum_tree): one-hot vectors (a wrong row mask or control drops or doubles a
    lane), magnitudes from 1e-8 to 1e8 in one wave, alternating signs, an inf in each row, a NaN in each lane in turn."""
    cases = dv.wave_sum_cases(np.random.default_rng(1))
    assert len(cases) * 64 % 256 == 0
    n = cases.size
    out = call('WAVE_SUM', [cases.reshape(-1)], [((n,), np.float32)], n, k0=block)[0]
    assert _same_word_per_wave(out.view(np.uint32))
    assert _equal_words(out.reshape(-1, 64)[:, 0], dv.wave_sum_ref(cases))
    assert np.array_equal(out.reshape(-1, 64)[:64, 0], np.ones(64, dtype=np.float32))          # the one-hot cases, spelled out
    lo, hi = call('WAVE_SUM_HALVES', [cases.reshape(-1)], [((n,), np.float32), ((n,), np.float32)], n, k0=block)
    assert _same_word_per_wave(lo.view(np.uint32)) and _same_word_per_wave(hi.view(np.uint32))
    rlo, rhi = dv.wave_sum_halves_ref(cases)
    assert _equal_words(lo.reshape(-1, 64)[:, 0], rlo) and _equal_words(hi.reshape(-1, 64)[:, 0], rhi)
    hot = np.arange(64)
    assert np.array_equal(lo.reshape(-1, 64)[:64, 0], (hot < 32).astype(np.float32))
    assert np.array_equal(hi.reshape(-1, 64)[:64, 0], (hot >= 32).astype(np.float32))


@pytest.mark.parametrize('block', [64, 256])
@pytest.mark.parametrize('largest', [True, False])
def test_wave_reduce_keys(largest, block):
    """wave_reduce<true> / <false> on uint64 keys: the extreme in each lane in turn, all equal, keys that differ in the low word
    only and in the high word only, high words ordered against the low words, 0 and all-ones present, random.  Every lane holds
    max / min of its wave's 64 keys."""
    cases = dv.wave_key_cases(np.random.default_rng(2), largest)
    assert len(cases) * 64 % 256 == 0
    n = cases.size
    out = call('WAVE_MAX' if largest else 'WAVE_MIN', [cases.reshape(-1)], [((n,), np.uint64)], n, k0=block)[0].reshape(-1, 64)
    ref = cases.max(axis=1) if largest else cases.min(axis=1)
    assert np.array_equal(out, np.repeat(ref[:, None], 64, axis=1))


def test_sort8_is_a_sorting_network():
    """sort8 on all 256 zero / one vectors (the 0-1 principle: a comparison network that sorts them sorts everything) and on 2^16
    random vectors of 16-bit ids padded with LIST_EMPTY: the output equals np.sort."""
    rng = np.random.default_rng(4)
    zero_one = (np.arange(256)[:, None] >> np.arange(8)[None, :] & 1).astype(np.uint32)
    ids = rng.integers(0, 0xFFFF, size=(1 << 16, 8)).astype(np.uint32)
    ids[np.arange(8)[None, :] >= rng.integers(0, 9, size=(1 << 16, 1))] = dv.LIST_EMPTY
    ids = rng.permuted(ids, axis=1)
    v = np.concatenate([zero_one, ids])
    out = call('SORT8', [v.reshape(-1)], [((v.size,), np.uint32)], len(v))[0].reshape(-1, 8)
    assert np.array_equal(out, np.sort(v, axis=1))


def test_obs_src_col_ordering():
    """obs_src_col(f, i) for every row i and every even column f in [0, 6N), N in {1, 2, 7}: own link first, then the others in agent
    order (obs_fn.py:43-53, restated in devfn_util.obs_src_col_ref)."""
    for N in (1, 2, 7):
        f, i = [a.reshape(-1).astype(np.uint32) for a in np.meshgrid(np.arange(0, 6 * N, 2), np.arange(N), indexing='ij')]
        got = call('OBS_SRC_COL', [f, i], [((len(f),), np.uint32)], len(f))[0]
        assert np.array_equal(got.astype(np.int64), dv.obs_src_col_ref(f, i)), N


SAME_RB_N = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 2048)
SAME_RB_R = (1, 2, 7, 256, 8192)


@pytest.mark.parametrize('R', SAME_RB_R)
def test_same_rb_sort_against_lexsort(R):
    """same_rb_keys / same_rb_rank / same_rb_starts staged as the kernels stage them (keys, barrier, rank, barrier, starts), one
    workgroup per env, THREADS = 256 (the one value csrc/ instantiates), for every N of SAME_RB_N and four envs each: random rb in
    [-2, R + 2), all on one RB, all out of range (INT_MIN and INT_MAX among them), one link per RB with empty RBs between.  The slots
    are the positions in np.lexsort((j, rb')), a permutation; every word of start[0 .. R] is written and is searchsorted's; the word
    behind start[R] keeps its sentinel."""
    rng = np.random.default_rng(R)
    for N in SAME_RB_N:
        rows = dv.same_rb_rows(rng, N, R)
        slot, start = call('SAME_RB', [rows.reshape(-1)], [((4, N), np.int32), ((4, R + 2), np.int32)], 4, k0=N, k1=R)
        for b in range(4):
            ref_slot, ref_start = dv.same_rb_ref(rows[b], R)
            assert np.array_equal(np.sort(slot[b]), np.arange(N)), (N, R, b)                   # a permutation
            assert np.array_equal(slot[b], ref_slot), (N, R, b)
            assert not np.any(start[b, :R + 1] == dv.SENTINEL), (N, R, b)                      # every word of start[0 .. R] written
            assert np.array_equal(start[b, :R + 1], ref_start), (N, R, b)
            assert start[b, R + 1] == dv.SENTINEL, (N, R, b)                                   # nothing behind start[R] touched
