"""No GPU: what was taken out of the fast time loop of step_kernel<8, 3, 1> is out of its machine code.

tests/test_gpu_step_diet.py pins the bytes, which would also hold if the compiler had put the work back into the loop.  This test
reads the three-barrier loop of the headline instance in the built library (disassembly and loop spans of tests/test_step_fast_isa.py):
  * no v_min_f64: the lane status is evaluated behind the loop, not in it (it was the loop's only use of fmin);
  * 22 v_cndmask_b32, against 44 in the loop before: the status took 24 (two came back with the hoisted chunk clamps).  What is
    left: one in the Poisson section, eighteen in the species section (sixteen for the last real row's missing super-diagonal, two
    for the first row's sub-diagonal) and three in the epilogue.
The test skips where the census tools are missing, as that file does.
"""
import re

from tests.test_step_fast_isa import disassembly, symbol      # noqa: F401  (disassembly: the module's fixture)

CNDMASK_BEFORE = 44
CNDMASK = 22


def fast_loop(ins):
    """Instructions of the widest backward-branch span with three barriers, row stores and no vector-memory load."""
    offsets = [o for o, _, _ in ins]
    best = []
    for k, (o, text, line) in enumerate(ins):
        m = re.search(r'<\w+\+0x([0-9a-f]+)>\s*$', line)
        if text.startswith(('s_cbranch', 's_branch')) and m and int(m.group(1), 16) <= o:
            body = [t for _, t, _ in ins[offsets.index(int(m.group(1), 16)):k + 1]]
            if (sum(t.startswith('s_barrier') for t in body) == 3 and sum(t.startswith('buffer_store') for t in body) >= 2 and
                    not any(t.startswith(('global_load', 'buffer_load', 'flat_load', 'scratch_load')) for t in body) and len(body) > len(best)):
                best = body
    return best


def test_status_and_its_selects_are_out_of_the_fast_loop(disassembly):      # noqa: F811
    body = fast_loop(disassembly[symbol(8, 3, 1)])
    assert len(body) >= 300, len(body)
    assert not any(t.startswith('v_min_f64') for t in body)
    n = sum(t.startswith('v_cndmask_b32') for t in body)
    print('v_cndmask_b32 in the fast loop:', n)
    assert n == CNDMASK and n < CNDMASK_BEFORE, n
