"""The step planner and the step kernels' names without a GPU, for the tests that name a kernel by its instantiation
(test_step_plan_cpu.py, test_table_route_cpu.py): tests/c/step_plan.cpp built as host code, the kernel names of a gfx950 code
object, and the mangled name of a `step_kernel<...>` / `rollout_kernel<...>` instantiation."""
import json
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def build_step_plan(directory):
    """Build tests/c/step_plan.cpp into `directory`; returns run(configs) -> one dict per configuration (plan or refusal)."""
    from gym_d2d_amd import build
    exe = Path(directory) / 'step_plan'
    cmd = [build._hipcc(), '-O1', '-std=c++17', '-Wall', '-x', 'hip', '--offload-host-only', '-I', str(build.INCLUDE),
           str(build.CSRC / 'd2d_plan.hip'), str(ROOT / 'tests' / 'c' / 'step_plan.cpp'), '-o', str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(configs):
        r = subprocess.run([str(exe), *configs], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return [json.loads(line) for line in r.stdout.splitlines()]
    return run


def kernel_names(tmp_path, source):
    """The d2d:: kernel names in the gfx950 code object of gym_d2d_amd/csrc/<source>, compiled in tmp_path."""
    from gym_d2d_amd import build
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / source), '-save-temps', '-o', 'k.o']
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp_path.glob('*gfx950*.s')).read_text()
    return set(re.findall(r'^\s+\.name:\s+(_ZN3d2d\w+)$', asm, flags=re.M))


def mangled(kernel):
    mode, *args = re.match(r'\w+<(.*)>', kernel).group(1).split(',')
    if kernel.startswith('rollout_kernel'):
        return f'_ZN3d2d14rollout_kernelILi{mode}ELi{args[0]}ELi{args[1]}EEEvNS_8StepArgsE'
    lpt, full, hot, opt = args
    return f'_ZN3d2d11step_kernelILi{mode}ELi{lpt}ELb{int(full == "true")}ELi{hot}ELi{opt}EEEvNS_8StepArgsE'
