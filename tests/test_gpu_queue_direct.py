"""Direct launches of d2d_queue_step (csrc/d2d_queue.hip: queue_step_kernel) past the parameters test_gpu_queue.py launches it at -
one link per env, no CUEs, a link count that is the workgroup, envs that straddle workgroups, packets of 2^25 - 1 bits in a buffer of
2^31 - 1 with budgets that saturate and 64 arrivals in a step, the step counter across 2^31 and at 2^32 - 1, the switch thresholds
at 0 and clipped to 2^32 - 1, a buffer smaller than a packet, the per-env clock fed by hand - bit for bit against the integer
restatement (queue_util.Restatement) on all eight planes and the ring after every launch.  The cases, each with the path it forces,
are queue_direct_util.CASES; test_element_direct_cpu.py asserts on the CPU that every case exercises what it claims (the event
counters, k = 64, a served x delay product above 2^32, a backlog beside 2^31).

Every launch reads and writes tensors this file builds.  The ring, the eight planes (and start_env under the per-env clock) lie inside
larger allocations with 4 KiB of a byte pattern before and after them; before the t = 0 launch they hold garbage (77, 12345, NaN);
after every launch the device is synchronised, the patterns are intact, the launch counter has moved by one and capacity_mbps,
elapsed_env, episode_env and reset_env are bit for bit what they were.

There is no tolerance: the model is integers but mean_delay_steps, one double division rounded once on both sides.

On one MI355X every case is equal at every launch; `limits` draws k = 64 five times, serves bits of age 31, holds 2 147 483 584 in a
plane and reaches a served x delay product of 2.07e10 (a 32-bit delay_sum fails it), wrap31 and wrap32 see 1 446 and 631 expiries
in their twelve far steps.  The 15 tests of this file took 4.4 s in all, the slowest 0.7 s (one_link, which also loads the library);
CHANGELOG.md has every case's event counts."""
from functools import lru_cache

import numpy as np
import pytest

import queue_direct_util as qdu
import queue_util as qu
from mobility_direct_util import CLOCK_B, clock_schedule

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from guard_util import Guarded, bits  # noqa: E402  (after the importorskip: it imports torch)

NAMES = qu.PLANES + ('ring',)


def _dtype(name):
    return torch.float32 if name == 'mean_delay_steps' else torch.uint8 if name == 'on' else torch.int32


class Launcher:
    """The guarded ring and planes of a case, full of garbage, and launch(): one d2d_queue_step with the checks every launch gets."""

    def __init__(self, name):
        self.name, self.s, self.c = name, qdu.spec(name), qdu.launch_constants(name)
        s = self.s
        self.arrays = {k: Guarded((s['b'], s['n']), _dtype(k)) for k in qu.PLANES}
        self.arrays['ring'] = Guarded((s['d'], s['b'], s['n']), torch.int32)
        for k, g in self.arrays.items():                              # garbage: t = 0 has to clear all of it
            g.array.fill_(float('nan') if k == 'mean_delay_steps' else 12345 if k == 'ring' else 77)
        self.capacity = torch.zeros((s['b'], s['n']), dtype=torch.float32, device='cuda')
        self.start = Guarded((s['b'],), torch.int32) if name == 'clock' else None
        self.launches = 0

    def get(self):
        return {k: g.array.cpu().numpy() for k, g in self.arrays.items()}

    def put(self, state):
        for k, g in self.arrays.items():
            g.array.copy_(torch.as_tensor(np.array(state[k]), device='cuda'))

    def launch(self, launch):
        from gym_d2d_amd import _native
        c, clock = self.c, launch['clock']
        self.capacity.copy_(torch.as_tensor(np.array(launch['capacity'])))
        kw, dev = dict(step=launch['step'], episode=launch['episode']), {}
        if clock is not None:
            dev = {k: torch.as_tensor(np.array(clock[k]).view(np.int32), device='cuda') for k in ('elapsed', 'episode', 'reset')}
            kw = dict(elapsed_ptr=dev['elapsed'].data_ptr(), start_ptr=self.start.array.data_ptr(), episode_ptr=dev['episode'].data_ptr(),
                      reset_ptr=dev['reset'].data_ptr())
        before = _native.queue_launches
        torch.cuda.synchronize()
        _native.queue_step(self.capacity.data_ptr(), self.arrays['ring'].array.data_ptr(),
                           *(self.arrays[k].array.data_ptr() for k in qu.PLANES), c['tables'], c['n_envs'], c['n_cues'], c['n_due_pairs'],
                           c['deadline_steps'], c['packet_bits'], c['buffer_bits'], c['bits_per_mbps_step'], *c['switches'], c['first_env'],
                           c['seed'], stream_ptr=torch.cuda.current_stream().cuda_stream, **kw)
        torch.cuda.synchronize()
        self.launches += 1
        what = f'{self.name} launch {self.launches}'
        assert _native.queue_launches == before + 1, what
        for k, g in self.arrays.items():
            assert g.intact(), f'{what}: bytes around {k} were written'
        if self.start is not None:
            assert self.start.intact(), f'{what}: bytes around start_env were written'
        assert np.array_equal(bits(self.capacity), bits(launch['capacity'])), f'{what}: capacity_mbps was written'
        for k, t in dev.items():
            assert np.array_equal(bits(t), bits(np.array(clock[k]))), f'{what}: {k}_env was written'

    def check(self, launch):
        got, what = self.get(), f'{self.name} launch {self.launches}'
        if launch['clock'] is None:
            what += f' (t = {launch["step"]})'
        for k in NAMES:
            w = launch['want'][k]
            assert got[k].shape == w.shape and got[k].dtype == w.dtype, (what, k)
            np.testing.assert_array_equal(bits(got[k]), bits(w), err_msg=f'{what}: {k}')


def test_the_package_s_plane_order_is_the_restatement_s():
    from gym_d2d_amd.queues import PLANES
    assert PLANES == qu.PLANES


@pytest.mark.parametrize('name', [n for n in qdu.CASES if n != 'clock'])
def test_lockstep_case_equals_the_restatement_bit_for_bit(name):
    launches, stats = qdu.program(name)
    s = qdu.spec(name)
    gpu = Launcher(name)
    for launch in launches:
        gpu.launch(launch)
        gpu.check(launch)
    print(f'{name} B={s["b"]} N={s["n"]} D={s["d"]}, t = 0 and {len(launches) - 1} steps ending at t = {launches[-1]["step"]}: every plane and the '
          f'ring equal; events {stats["events"]}, oldest served age {stats["max_served_age"]}, k = 64 draws {stats["k64"]}, largest plane '
          f'value {stats["max_plane"]}, largest served x delay {stats["max_product"]:.3g}')
    # a second episode clears what the first left
    ref = qdu.restatement(name).start(s['episode'] + 1 & 0xFFFFFFFF)
    again = dict(step=0, episode=s['episode'] + 1 & 0xFFFFFFFF, capacity=launches[0]['capacity'], want=ref.planes(), clock=None)
    gpu.launch(again)
    gpu.check(again)


def test_a_second_launch_from_the_same_state_gives_the_same_bytes():
    launches, _ = qdu.program('limits')
    k = 60
    gpu = Launcher('limits')
    for _ in range(2):
        gpu.put(launches[k - 1]['want'])
        gpu.launch(launches[k])
        gpu.check(launches[k])


@lru_cache(maxsize=None)
def _run_clock():
    """The 31 launches of the clock case; start_env as every launch left it."""
    launches, stats = qdu.program('clock')
    gpu = Launcher('clock')
    starts = []
    for k, launch in enumerate(launches, start=1):
        if k <= 2:                                                    # garbage, then the stagger; afterwards what the kernel left
            gpu.start.array.copy_(torch.as_tensor(np.array(launch['clock']['start'])))
        assert np.array_equal(gpu.start.array.cpu().numpy(), launch['clock']['start']), k
        gpu.launch(launch)
        gpu.check(launch)
        starts.append(gpu.start.array.cpu().numpy())
    return starts, stats


def test_per_env_clock_equals_one_single_env_restatement_per_env():
    starts, stats = _run_clock()
    assert len(starts) == 31
    print(f'clock B={CLOCK_B} N=131 D=32, 31 launches: every plane and the ring equal at every launch; events {stats["events"]}, oldest '
          f'served age {stats["max_served_age"]}')


def test_per_env_clock_writes_start_env_of_flagged_envs_and_of_no_other():
    starts, _ = _run_clock()
    for k, (launch, start) in enumerate(zip(clock_schedule(), starts), start=1):
        assert start.dtype == np.int32 and np.array_equal(start, launch['start_after']), k
