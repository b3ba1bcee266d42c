"""What test_gpu_devfn.py rests on, checked without a GPU: its references against independent ones, the functions' arithmetic as
written (emulated in NumPy float32 with correctly rounded log2 / exp2) against the figures the headers state, the wrapper source's
promise to define nothing it tests, the entry point's refusals, and the build table."""
import math
import re

import numpy as np
import pytest

import devfn_util as dv
import test_gpu_devfn as gpu
from gym_d2d_amd import build
from oracle import d2d_oracle as orc

HEADER = (dv.CSRC / 'd2d_step_device.h').read_text()


def test_the_asserted_figures_are_the_headers():
    """Each bound test_gpu_devfn.py asserts is the figure the function's comment in d2d_step_device.h states."""
    for text, constant, figure in (('to 2.7e-7 relative', gpu.POW_NEG_HALF_REL, 2.7e-7), ('(dBm -> mW), ~1.5e-7 relative', gpu.POW10_TENTH_REL, 1.5e-7),
                                   ('// 6.9e-7 relative in all', gpu.POW_K_REL, 6.9e-7), ('division sequence (~10 VALU): 2e-7 relative', gpu.FAST_DIV_REL, 2e-7),
                                   ('x / y to within an ulp', gpu.PRECISE_DIV_ULP, 1), ('Box-Muller to 5.6e-7 absolute in z', gpu.PHILOX_NORMAL_ABS, 5.6e-7),
                                   ('1.07e-7 absolute at worst over all 2^24 arguments', gpu.COS_TURNS_ABS, 1.07e-7)):
        assert text in HEADER and constant == figure, text
    assert gpu.PRECISE_DIV_ULP == 1 and 2.0 * gpu.COS_TURNS_ABS <= gpu.COS_TURNS_CAP == 2.0 ** -22


# ------------------------------------------------------------------------------------------------ the references check themselves
def test_the_tree_restatement_sums_and_depends_on_the_order():
    """wave_sum_tree equals math.fsum within 64 ulp on benign input (it IS a sum of the 64 lanes), and two orders of the same data
    give different words on the mixed-magnitude input (else the GPU test would prove nothing about the order of the additions)."""
    rng = np.random.default_rng(0)
    benign = rng.uniform(1.0, 2.0, size=(256, 64)).astype(np.float32)
    exact = np.array([math.fsum(map(float, row)) for row in benign])
    got = dv.wave_sum_ref(benign)
    assert np.all(np.abs(got.astype(np.float64) - exact) <= 64 * np.spacing(exact.astype(np.float32)).astype(np.float64))
    lo, hi = dv.wave_sum_halves_ref(benign)
    assert np.array_equal(lo + hi, got)                                   # the sixth level adds the two halves, in one addition
    tree = dv.wave_sum_tree(benign)
    assert np.array_equal(tree[:, 48:], np.repeat(got[:, None], 16, axis=1))                # row 3 holds the total in every lane
    hot = np.eye(64, dtype=np.float32)
    assert np.array_equal(dv.wave_sum_ref(hot), np.ones(64, dtype=np.float32))
    lo, hi = dv.wave_sum_halves_ref(hot)
    assert np.array_equal(lo, (np.arange(64) < 32).astype(np.float32)) and np.array_equal(hi, (np.arange(64) >= 32).astype(np.float32))
    mixed = dv.wave_sum_cases(np.random.default_rng(1))[64:128]
    assert np.all(np.isfinite(mixed)) and mixed.max() / mixed.min() > 1e12
    rolled = np.roll(mixed, 5, axis=1)
    assert np.mean(dv.f32_bits(dv.wave_sum_ref(mixed)) != dv.f32_bits(dv.wave_sum_ref(rolled))) > 0.25
    assert np.array_equal(np.sort(mixed, axis=1), np.sort(rolled, axis=1))


def test_wave_key_cases_hold_what_they_name():
    for largest in (True, False):
        cases = dv.wave_key_cases(np.random.default_rng(2), largest)
        hot = cases[:64]
        assert np.array_equal(hot.argmax(axis=1) if largest else hot.argmin(axis=1), np.arange(64))
        assert np.array_equal((cases[64:128].argmax(axis=1) if largest else cases[64:128].argmin(axis=1)), np.arange(64))
        low, high, opposite, ends = cases[136:152], cases[152:168], cases[168:184], cases[184:200]
        assert np.all(low >> np.uint64(32) == low[:, :1] >> np.uint64(32)) and np.all(high << np.uint64(32) == high[:, :1] << np.uint64(32))
        hi, lo = (opposite >> np.uint64(32)).astype(np.int64), (opposite & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert np.array_equal(np.argsort(hi, axis=1), np.argsort(-lo, axis=1))
        assert np.all(ends.min(axis=1) == 0) and np.all(ends.max(axis=1) == np.uint64(0xFFFFFFFFFFFFFFFF))


def test_head_tail_reconstructs_the_exponent():
    """head + tail is -e / 2 to half an ulp of a float32 tail: the head keeps 12 significant bits of a value in [1, 2.3], so what is
    left is below 2^-10 and its float32 rounding below 2^-35 (d2d_capi.hip: "the pair carries ~36 bits"); 2^-34 is asserted, the
    exponents a float32 pair holds exactly (the fixed set's 2, 2.5, 3, 3.5, 4) to 0.  head * fe is exact for every binary exponent."""
    _, e = dv.pow_neg_half_inputs()
    head, tail = dv.head_tail(e)
    back = head.astype(np.float64) + tail.astype(np.float64)
    assert np.abs(back - (-0.5 * e)).max() < 2.0 ** -34
    exact = np.isin(e, (2.0, 2.5, 3.0, 3.5, 4.0))
    assert np.all(back[exact] == -0.5 * e[exact]) and np.all(tail[exact] == 0.0)
    assert np.all(dv.f32_bits(head) & np.uint32(0xFFF) == 0) and np.all(np.abs(tail) < 2.0 ** -10)
    for fe in (-149.0, -5.0, 41.0, 128.0):
        assert np.all((head * np.float32(fe)).astype(np.float64) == head.astype(np.float64) * fe)


def test_the_lexsort_reference_is_a_rank_count():
    rng = np.random.default_rng(9)
    for N in (1, 3, 4, 5, 63, 64, 65):
        for R in (1, 2, 7, 256):
            for row in dv.same_rb_rows(rng, N, R):
                slot, start = dv.same_rb_ref(row, R)
                eff = [int(r) if 0 <= r < R else R for r in row]
                brute = [sum((eff[k], k) < (eff[j], j) for k in range(N)) for j in range(N)]
                assert list(slot) == brute
                assert list(start) == [sum(x < r for x in eff) for r in range(R + 1)]
    rows = dv.same_rb_rows(rng, 5, 256)
    assert rows[2].min() == -2 ** 31 and rows[2].max() == 2 ** 31 - 1 and len(set(rows[1])) == 1 and len(set(rows[3])) == 5


def test_the_obs_column_reference_is_the_oracle_expansion():
    for N in (1, 2, 7):
        table = np.arange(6 * N, dtype=np.float64).reshape(1, N, 6) + 100.0
        obs = orc.expand_obs(table)[0]
        f, i = np.meshgrid(np.arange(6 * N), np.arange(N), indexing='ij')
        assert np.array_equal(obs[i, f], table.reshape(-1)[dv.obs_src_col_ref(f, i)])


# ------------------------------------------------------------------------------------------------ the arithmetic as written
def test_pow10_tenth_as_written_stays_inside_its_figure():
    """The split's own error with a correctly rounded exp2: 7.1e-8 on p in [-379, 385]; an edit that breaks the head / tail constants
    shows here without a GPU."""
    p = np.arange(-379, 386)
    err = dv.rel_err(dv.emulate_pow10_tenth(p), 10.0 ** (p / 10.0))
    print(f'pow10_tenth as written: {err.max():.3e}')
    assert err.max() <= 7.2e-8 < gpu.POW10_TENTH_REL
    wide = dv.emulate_pow10_tenth(np.arange(-4095, 4096))
    assert np.all(np.diff(wide.astype(np.float64)[np.isfinite(wide)]) >= 0.0)


def test_pow_neg_half_as_written_stays_inside_its_figure():
    """The same for pow_neg_half on the whole domain of the GPU test: 2.2e-7."""
    d2, e = dv.pow_neg_half_inputs()
    head, tail = dv.head_tail(e)
    err = dv.rel_err(dv.emulate_pow_neg_half(d2, head, tail), np.power(d2.astype(np.float64), -0.5 * e))
    print(f'pow_neg_half as written: {err.max():.3e}')
    assert err.max() <= gpu.POW_NEG_HALF_REL


# ------------------------------------------------------------------------------------------------ the wrapper source and the entry point
def test_the_wrapper_source_defines_nothing_it_tests():
    text = (dv.CSRC / 'd2d_devfn.hip').read_text()
    for header in ('d2d_step_device.h', 'd2d_wave_key.h', 'd2d_same_rb.h'):
        assert f'#include "{header}"' in text
    for name in dv.TESTED:
        assert name + '(' in text or name + '<' in text or name in ('dpp_key', 'dpp_f32'), name          # ... and calls each
        assert not re.search(r'\b' + name + r'\s*(<[^;{}()]*>)?\s*\([^;{}]*\)\s*(const\s*)?\{', text), name
    assert '#define' not in text and 'asm' not in text and 'atomic' not in re.sub(r'//.*', '', text)


def test_the_same_rb_wrapper_is_instantiated_as_the_kernels_are():
    """Every kernel of csrc/ that stages the same-RB sort instantiates it with one THREADS value, and the wrapper with the same."""
    values = set()
    for src in dv.CSRC.glob('*.hip'):
        text = src.read_text()
        for name in set(re.findall(r'same_rb_(?:keys|starts)<(\w+)', text)):
            if src.name != 'd2d_devfn.hip' or name != 'THREADS':
                values.add(int(re.search(rf'constexpr int {name} = (\d+);', text).group(1)))
    assert values == {256}
    assert 'constexpr int SAME_RB_THREADS = 256;' in (dv.CSRC / 'd2d_devfn.hip').read_text()


REFUSALS = [
    (dict(fn=-1), 'unknown fn'), (dict(fn=dv.FN_COUNT), 'unknown fn'),
    (dict(fn='COS_TURNS', a=16, out0=16, n=-1), 'n must not be negative'),
    (dict(fn='COS_TURNS', a=16, out0=16, n=1 << 31), 'n must be below 2^31'),
    (dict(fn='COS_TURNS', out0=16, n=4), 'null device pointer: a'),
    (dict(fn='COS_TURNS', a=16, n=4), 'null device pointer: out0'),
    (dict(fn='COS_TURNS', a=16, n=0), 'null device pointer: out0'),
    (dict(fn='POW_NEG_HALF', a=16, b=16, out0=16, n=4), 'null device pointer: c'),
    (dict(fn='PRECISE_DIV', a=16, out0=16, n=4), 'null device pointer: b'),
    (dict(fn='PHILOX_STEP', a=16, b=16, out0=16, n=4), 'null device pointer: out1'),
    (dict(fn='WAVE_SUM_HALVES', a=16, out0=16, n=64, k0=64), 'null device pointer: out1'),
    (dict(fn='SAME_RB', a=16, out0=16, n=1, k0=4, k1=4), 'null device pointer: out1'),
    (dict(fn='WAVE_SUM', a=16, out0=16, n=100, k0=64), 'n must be a multiple of the block'),
    (dict(fn='WAVE_SUM_HALVES', a=16, out0=16, out1=16, n=64, k0=256), 'n must be a multiple of the block'),
    (dict(fn='WAVE_MAX', a=16, out0=16, n=63, k0=64), 'n must be a multiple of the block'),
    (dict(fn='WAVE_MIN', a=16, out0=16, n=128, k0=128), 'the block (k0) must be 64 or 256'),
    (dict(fn='WAVE_SUM', a=16, out0=16, n=128, k0=0), 'the block (k0) must be 64 or 256'),
    (dict(fn='SAME_RB', a=16, out0=16, out1=16, n=1, k0=0, k1=4), 'N (k0) must be in [1, 2048]'),
    (dict(fn='SAME_RB', a=16, out0=16, out1=16, n=1, k0=dv.MAX_LINKS + 1, k1=4), 'N (k0) must be in [1, 2048]'),
    (dict(fn='SAME_RB', a=16, out0=16, out1=16, n=1, k0=4, k1=0), 'R (k1) must be in [1, 8192]'),
    (dict(fn='SAME_RB', a=16, out0=16, out1=16, n=1, k0=4, k1=dv.MAX_RBS + 1), 'R (k1) must be in [1, 8192]'),
    (dict(fn='POW_K_GAINS', a=16, b=16, out0=16, n=4, k0=0), 'pow_k must be in [1, 8]'),
    (dict(fn='POW_K_GAINS', a=16, b=16, out0=16, n=4, k0=9), 'pow_k must be in [1, 8]'),
    (dict(fn='POW_K_GAINS', a=16, b=16, out0=16, n=4, k0=4, k1=3), 'the form (k1) must be 0, 1 or 2'),
    (dict(fn='POW_K_GAINS', a=16, b=16, out0=16, n=4, k0=3, k1=2), 'form 2 is compiled for k == 4'),
    (dict(fn='PAIR_GAIN', a=16, b=16, c=16, out0=16, n=4, k0=2), 'the mode (k0) must be 0, 1 or 4'),
    (dict(fn='PAIR_GAIN', a=16, b=16, c=16, out0=16, n=4, k0=dv.PL_POWK, k1=0), 'pow_k must be in [1, 8]'),
    (dict(fn='PAIR_GAIN', a=16, b=16, c=16, out0=16, n=4, k0=dv.PL_POWK, k1=9), 'pow_k must be in [1, 8]'),
]


@pytest.mark.parametrize('kwargs, text', REFUSALS, ids=[f'{k}-{t}' for k, (_, t) in enumerate(REFUSALS)])
def test_the_entry_point_refuses_by_name_without_a_launch(kwargs, text):
    """Every refusal comes before the launch: this machine has no GPU to launch on, and the pointers are not memory."""
    with pytest.raises(ValueError) as e:
        dv.device_fn(**kwargs)
    assert text in str(e.value) and str(e.value).startswith('d2d_probe_device_fn')
    if isinstance(kwargs['fn'], str):
        assert str(e.value).startswith('d2d_probe_device_fn(')                         # ... and names the function


def test_nothing_to_do_is_accepted_without_a_launch():
    for name in dv.FN:
        k0, k1 = {'WAVE_SUM': (64, 0), 'WAVE_SUM_HALVES': (256, 0), 'WAVE_MAX': (64, 0), 'WAVE_MIN': (256, 0), 'SAME_RB': (2048, 8192),
                  'POW_K_GAINS': (4, 2), 'PAIR_GAIN': (dv.PL_POWK, 8)}.get(name, (0, 0))
        dv.device_fn(name, 16, 16, 16, 16, 16, n=0, k0=k0, k1=k1)
    assert len(dv.FN) == dv.FN_COUNT and sorted(dv.FN.values()) == list(range(dv.FN_COUNT))
    diag = (dv.ROOT / 'include' / 'd2d_hip_diag.h').read_text()
    for name, k in dv.FN.items():
        assert re.search(rf'D2D_DEVFN_{name} = {k},', diag), name
    assert f'D2D_DEVFN_COUNT = {dv.FN_COUNT}' in diag and f'#define D2D_DEVFN_SENTINEL 0x{dv.SENTINEL:X}' in diag


def test_the_probe_library_has_two_sources_and_both_are_hashed():
    assert build.LIBRARIES['probe'] == ['d2d_probe.hip', 'd2d_devfn.hip']
    hashed = [p.name for p in build.digest_files()]
    assert 'd2d_probe.hip' in hashed and 'd2d_devfn.hip' in hashed
    for header in ('d2d_step_device.h', 'd2d_wave_key.h', 'd2d_same_rb.h', 'd2d_hip_diag.h'):
        assert header in hashed
