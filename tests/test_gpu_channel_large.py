"""Direct launches of d2d_channel_fill (csrc/d2d_channel.hip: channel_phase_kernel + channel_fill_kernel) past the shapes
test_gpu_channel.py reaches through VecD2DEnv - 9 to 17 envs, 64 to 2048 links, 65535 devices, the env counter at 2^32 - 1, the
per-env clock over two groups of eight - against the float64 restatement of include/d2d_channel.h with explicit per-device columns
(channel_util.table_db_columns).  The cases, each with the path it forces, are channel_large_util.CASES; test_channel_cpu.py asserts
on the CPU that the restatement can judge them and that they cover what they claim.

Every launch reads and writes tensors this file builds.  table, phase_scratch, start_env, pos_x and pos_y lie inside larger
allocations with 4 KiB of a byte pattern before and after them, table and phase_scratch are NaN before the launch; after it the
patterns are intact, no NaN is left, and every input is bit for bit what it was.

Measured on one MI355X (worst |got - want| / |want| over the kept entries; the bar is 1e-5; share left out as deep fades):
    a  float32  9 x   64 links, M_s  8, Rayleigh   9.2e-8   5.3e-5
    b  float64 17 x   65 links, M_s 16, Rician     1.7e-7   0
    c  float64 11 x  259 links, M_s 32, Rayleigh   9.2e-8   6.5e-5      float32: 1.1e-7
    d  float32  2 x 1030 links, M_s  8, Rician     5.1e-7   5.2e-6
    e  float64  1 x 2048 links, M_s  8, Rayleigh   8.1e-8   2.5e-5
    f  float64  9 x   70 links, 65535 devices      7.7e-8   4.5e-5 (Rayleigh)      1.4e-7, 0 (Rician)
    g  no shadowing, no fading, 9 x 131 links      6.3e-8 (float32)   1.3e-8 (float64)
    h  g with one entry of -inf                    as g; the entry is -inf in both widths
The 22 tests of this file took about 2.4 s in all, the slowest 0.70 s (case a, which also loads the library); CHANGELOG.md has the rest."""
from functools import lru_cache

import numpy as np
import pytest

import channel_large_util as clu
import channel_util as cu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

GUARD = 4096
PARAMS = [(name, dtype) for name, spec in clu.CASES.items() for dtype in spec['dtypes']]
BOTH_WIDTHS = [name for name, spec in clu.CASES.items() if len(spec['dtypes']) == 2]


class Guarded:
    """A device array of `shape` and `dtype` inside a larger allocation: GUARD bytes of a pattern before and after it."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        total = 2 * GUARD + self.nbytes
        self.pattern = ((torch.arange(total, dtype=torch.int64, device='cuda') * 7 + 3) % 251).to(torch.uint8)
        self.buf = self.pattern.clone()
        self.array = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        assert self.array.data_ptr() % 16 == 0 and self.array.data_ptr() == self.buf.data_ptr() + GUARD

    def intact(self):
        lo, hi = slice(0, GUARD), slice(GUARD + self.nbytes, None)
        return bool(torch.equal(self.buf[lo], self.pattern[lo])) and bool(torch.equal(self.buf[hi], self.pattern[hi]))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _launch(name, dtype, lo=0, hi=None):
    """One d2d_channel_fill of the envs [lo, hi) of a case into a fresh NaN table; the guard, NaN and input checks every launch
    gets; returns (table as NumPy, start_env after the launch or None)."""
    from gym_d2d_amd import _native
    c = clu.build_case(name)
    hi = c['b'] if hi is None else hi
    b, n, d, m = hi - lo, c['n'], c['d'], c['m']
    tdtype = torch.float64 if dtype == 'float64' else torch.float32
    pos_x, pos_y = Guarded((b, d), torch.float32), Guarded((b, d), torch.float32)
    pos_x.array.copy_(torch.as_tensor(np.ascontiguousarray(c['pos'][lo:hi, :, 0])))
    pos_y.array.copy_(torch.as_tensor(np.ascontiguousarray(c['pos'][lo:hi, :, 1])))
    table = Guarded((b, n + 1, n), tdtype)
    table.array.fill_(float('nan'))
    scratch = Guarded((b, n, m, 4), torch.float32) if m else None
    if scratch is not None:
        scratch.array.fill_(float('nan'))
    inputs = {k: np.array(c[k]) for k in ('tx', 'rx', 'a_tx', 'a_rx', 'expo')}
    guarded = {'pos_x': pos_x, 'pos_y': pos_y, 'table': table}
    clock, start = dict(step=clu.T, episode=clu.EPISODE), None
    if c['clock'] is not None:
        k = c['clock']
        start = Guarded((b,), torch.int32)
        start.array.copy_(torch.as_tensor(np.array(k['start'][lo:hi])))
        guarded['start_env'] = start
        inputs.update(elapsed=np.array(k['elapsed'][lo:hi]), episode=np.array(k['episode'][lo:hi]).view(np.int32),
                      reset=np.array(k['reset'][lo:hi]))
    if scratch is not None:
        guarded['phase_scratch'] = scratch
    dev = {k: torch.as_tensor(v, device='cuda') for k, v in inputs.items()}
    if c['clock'] is not None:
        clock = dict(elapsed_ptr=dev['elapsed'].data_ptr(), start_ptr=start.array.data_ptr(), episode_ptr=dev['episode'].data_ptr(),
                     reset_ptr=dev['reset'].data_ptr())
    m_s, amp, wave_scale, fading, mu, s = cu.constants(clu.SHADOW_STD_DB if m else 0.0, clu.DECORRELATION_M, m or 16, c['fading'],
                                                       clu.RICIAN_K_DB)
    assert m_s == m
    shadow_seed, fading_seed = clu.seeds()
    torch.cuda.synchronize()
    _native.channel_fill(pos_x.array.data_ptr(), pos_y.array.data_ptr(), dev['tx'].data_ptr(), dev['rx'].data_ptr(),
                         dev['a_tx'].data_ptr(), dev['a_rx'].data_ptr(), dev['expo'].data_ptr(), b, d, n, c['first_env'] + lo, m, amp,
                         wave_scale, fading, mu, s, shadow_seed, fading_seed, scratch.array.data_ptr() if m else 0,
                         table.array.data_ptr(), _native.F64 if dtype == 'float64' else _native.F32, **clock)
    torch.cuda.synchronize()
    for what, g in guarded.items():
        assert g.intact(), f'{name} {dtype}: bytes around {what} were written'
    for what, want in inputs.items():
        assert np.array_equal(_bits(dev[what].cpu().numpy()), _bits(want)), f'{name} {dtype}: {what} was written'
    assert np.array_equal(_bits(pos_x.array.cpu().numpy()), _bits(c['pos'][lo:hi, :, 0])), f'{name} {dtype}: pos_x was written'
    assert np.array_equal(_bits(pos_y.array.cpu().numpy()), _bits(c['pos'][lo:hi, :, 1])), f'{name} {dtype}: pos_y was written'
    got = table.array.cpu().numpy()
    assert got.dtype == np.dtype(dtype) and got.shape == (b, n + 1, n)
    holes = np.argwhere(np.isnan(got))
    assert len(holes) == 0, f'{name} {dtype}: {len(holes)} entries are NaN (not written, or NaN), the first at {holes[0].tolist()}'
    if scratch is not None:
        assert not bool(torch.isnan(scratch.array).any()), f'{name} {dtype}: phase_scratch has words the phase kernel did not write'
    return got, None if start is None else start.array.cpu().numpy()


@lru_cache(maxsize=None)
def _whole(name, dtype):
    """The whole batch of a case, launched once and shared by the tests."""
    got, start = _launch(name, dtype)
    got.setflags(write=False)
    return got, start


# ------------------------------------------------------------------------------------------ 1: entry by entry
@pytest.mark.parametrize('name,dtype', PARAMS)
def test_table_matches_the_column_restatement_entry_by_entry(name, dtype):
    """The existing measure and bars (channel_util.entry_error, TOL, DEEP_FADE, DEEP_FADE_CAP); row N is the diagonal bit for bit;
    an entry is -inf exactly where the restatement's is (case h: one transmitter on another link's receiver, log10 0)."""
    c = clu.build_case(name)
    want, h2 = clu.restated(name)
    got, _ = _whole(name, dtype)
    n = c['n']
    inf = clu.infinite_entries(c)
    assert np.array_equal(np.isneginf(got), inf) and not np.isposinf(got).any()
    err, left_out = cu.entry_error(got, want, h2, inf)
    print(f'{name} {dtype} B={c["b"]} N={n} D={c["d"]} M_s={c["m"]} {c["fading"]}: worst error {err:.3g} of the entry, '
          f'{left_out:.2g} left out')
    assert left_out <= cu.DEEP_FADE_CAP
    assert err <= cu.TOL
    assert np.array_equal(_bits(got[:, n]), _bits(got[:, np.arange(n), np.arange(n)]))


# ------------------------------------------------------------------------------------------ 2: bit for bit
@pytest.mark.parametrize('name', BOTH_WIDTHS)
def test_float32_entries_are_the_float64_entries_rounded_once(name):
    wide, narrow = _whole(name, 'float64')[0], _whole(name, 'float32')[0]
    assert (wide != wide.astype(np.float32)).any()                   # the float64 entries carry more than float32
    assert np.array_equal(_bits(wide.astype(np.float32)), _bits(narrow))


@pytest.mark.parametrize('dtype', clu.CASES['c']['dtypes'])
def test_per_env_clock_zeroes_start_env_of_pending_envs_and_no_other(dtype):
    k = clu.build_case('c')['clock']
    _, start = _whole('c', dtype)
    assert start.dtype == np.int32
    assert np.array_equal(start, np.where(k['reset'] != 0, 0, k['start']))
    assert (k['start'][k['reset'] != 0] != 0).any()                  # some pending env had something to lose


@pytest.mark.parametrize('name,dtype', [(name, dtype) for name in clu.SHARDS for dtype in clu.CASES[name]['dtypes']])
def test_a_shard_across_two_groups_of_eight_equals_the_whole_batch(name, dtype):
    """Envs [lo, hi) with first_env + lo, sliced position planes and sliced clock arrays, into a fresh table."""
    lo, hi = clu.SHARDS[name]
    whole, whole_start = _whole(name, dtype)
    part, part_start = _launch(name, dtype, lo, hi)
    assert np.array_equal(_bits(part), _bits(whole[lo:hi]))
    if whole_start is not None:
        assert np.array_equal(part_start, whole_start[lo:hi])


@pytest.mark.parametrize('name', ['f_rayleigh', 'f_rician'])
def test_links_of_one_device_share_columns_and_rows(name):
    """Keyed by DEVICE pair: links with one receiver device hold equal columns (rows 0 .. N-1; row N is each link's own diagonal),
    links with one transmitter device equal rows."""
    c = clu.build_case(name)
    got, n = _whole(name, 'float64')[0], c['n']
    cols, rows = got[:, :n, clu.SHARED_RX], got[:, clu.SHARED_TX, :]
    assert cols.shape[2] >= 2 and rows.shape[1] >= 2
    assert np.array_equal(_bits(cols), _bits(np.repeat(cols[:, :, :1], cols.shape[2], axis=2)))
    assert np.array_equal(_bits(rows), _bits(np.repeat(rows[:, :1], rows.shape[1], axis=1)))
    assert not np.array_equal(got[:, :n, clu.SHARED_RX.start], got[:, :n, clu.SHARED_RX.stop])
    assert not np.array_equal(got[:, clu.SHARED_TX.start], got[:, clu.SHARED_TX.stop])
