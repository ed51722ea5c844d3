"""No GPU: the machine code of step_kernel<P, W, G> in the built library holds the two bodies the source promises.

tests/test_gpu_step_fast.py compares the fast body with the general one bit for bit, which would also pass if the kernel never chose
the fast body or if the fast body were compiled without what makes it fast.  This test reads the gfx950 code object of the built
library and checks, for the headline instance step_kernel<8, 3, 1> and for one instance per other points-per-lane value:
  * the kernel holds a time loop with exactly three workgroup barriers, no vector-memory load and no wait on the vector-memory
    counter (the fast body's steady state: rows resident in LDS, launch constants in scalar registers), and
  * it also holds a loop with four or more barriers and vector-memory loads (the general body),
and that an instance kept on the general body alone (P = 1, and <2, 1, 3>) has no loop of the first kind.  Which of the two a launch
runs is one scalar test of kernel arguments in front of both; the counters of profiles/step_fast_bench.md show the fast one running.
"""
import os
import re
import subprocess
import tempfile

import pytest

from tests import kernel_census as K


def symbol(P, W, G):
    return '_ZN3pnp11step_kernelILi%dELi%dELi%dEEEvNS_7DevArgsE' % (P, W, G)


@pytest.fixture(scope='module')
def disassembly():
    """{symbol: [(offset, text)]} of the step_kernel instances named below (one objdump call on the object that holds them)."""
    syms = [symbol(*k) for k in ((8, 3, 1), (2, 2, 1), (4, 1, 3), (16, 3, 1), (1, 3, 1), (2, 1, 3))]
    try:
        objcopy, bundler, objdump = K._tool('llvm-objcopy'), K._tool('clang-offload-bundler'), K._tool('llvm-objdump')
        if not os.path.exists(K.LIB):
            raise K.CensusUnavailable('the library is not built')
    except K.CensusUnavailable as e:
        pytest.skip(str(e))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, 'fatbin')
        subprocess.run([objcopy, '--dump-section', '.hip_fatbin=' + fat, K.LIB, os.path.join(tmp, 'copy.so')], check=True, capture_output=True)
        with open(fat, 'rb') as f:
            bundles = K.split_bundles(f.read())
        for k, blob in enumerate(bundles):
            src, obj = os.path.join(tmp, 'b%d' % k), os.path.join(tmp, 'o%d' % k)
            with open(src, 'wb') as f:
                f.write(blob)
            subprocess.run([bundler, '--unbundle', '--type=o', '--targets=' + K.TARGET, '--input=' + src, '--output=' + obj,
                            '--allow-missing-bundles'], check=True, capture_output=True)
            if not os.path.exists(obj) or os.path.getsize(obj) == 0:
                continue
            r = subprocess.run([objdump, '-d', '--disassemble-symbols=' + ','.join(syms), obj], check=True, capture_output=True, text=True)
            cur = None
            for line in r.stdout.splitlines():
                m = re.match(r'^[0-9a-f]+ <(\w+)>:', line)
                if m:
                    cur = out.setdefault(m.group(1), []) if m.group(1) in syms else None
                    base = int(line.split()[0], 16)
                    continue
                m = re.match(r'^\s+(\S.*?)\s+// ([0-9A-F]+):', line)
                if m and cur is not None:
                    cur.append((int(m.group(2), 16) - base, m.group(1), line))
    assert set(out) == set(syms), sorted(set(syms) - set(out))
    return out


def loops(ins):
    """Instruction mix of the span [target, branch] of every backward branch of a kernel."""
    offsets = [o for o, _, _ in ins]
    out = []
    for k, (o, text, line) in enumerate(ins):
        m = re.search(r'<\w+\+0x([0-9a-f]+)>\s*$', line)
        if text.startswith(('s_cbranch', 's_branch')) and m and int(m.group(1), 16) <= o:
            body = [t for _, t, _ in ins[offsets.index(int(m.group(1), 16)):k + 1]]
            out.append({'n': len(body), 'barriers': sum(t.startswith('s_barrier') for t in body),
                        'loads': sum(t.startswith(('global_load', 'buffer_load', 'flat_load', 'scratch_load')) for t in body),
                        'vmcnt': sum(t.startswith('s_waitcnt') and 'vmcnt' in t for t in body),
                        'row_stores': sum(t.startswith('buffer_store') for t in body)})
    return out


def time_loops(ins):
    """The spans that hold a whole timestep: they store the rows and the charge row (buffer stores of a row and of the charge row, hundreds of instructions)."""
    return [m for m in loops(ins) if m['row_stores'] >= 2 and m['n'] >= 300]


@pytest.mark.parametrize('P,W,G', [(8, 3, 1), (2, 2, 1), (16, 3, 1)])
def test_instance_holds_a_resident_loop_and_a_general_loop(P, W, G, disassembly):
    found = time_loops(disassembly[symbol(P, W, G)])
    assert any(m['barriers'] == 3 and m['loads'] == 0 and m['vmcnt'] == 0 for m in found), found
    assert any(m['barriers'] >= 4 and m['loads'] > 0 for m in found), found


def test_single_wave_instance_holds_a_loop_without_loads(disassembly):
    """W = 1: the workgroup hand-offs are wave-level (no s_barrier), so only the loads tell the two bodies apart."""
    found = time_loops(disassembly[symbol(4, 1, 3)])
    assert any(m['loads'] == 0 and m['vmcnt'] == 0 for m in found), found
    assert any(m['loads'] > 0 for m in found), found


@pytest.mark.parametrize('P,W,G', [(1, 3, 1), (2, 1, 3)])
def test_instances_left_on_the_general_body(P, W, G, disassembly):
    found = time_loops(disassembly[symbol(P, W, G)])
    assert found and all(m['loads'] > 0 for m in found), found
