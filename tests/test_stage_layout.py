"""The layout of the staged inputs and output rows of an entry point (catint_amd/csrc/pnp_stage.h), tested on the host: the header has
no HIP dependency, so tests/csrc/stage_check.cpp is compiled against it alone with g++ and run.  The program asserts that inputs of
mixed sizes start at even offsets in declaration order without overlap, that `place` writes exactly the declared members, that an input
left undeclared keeps its null, that the declarations of catcpl_solve and of the microkinetic libraries reproduce the offset chains
they replaced (restated there literally), and that rows_doubles and place_rows agree."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'catint_amd', 'csrc')
SOURCE = os.path.join(ROOT, 'tests', 'csrc', 'stage_check.cpp')


def test_the_header_has_no_hip_dependency():
    text = open(os.path.join(CSRC, 'pnp_stage.h')).read()
    includes = sorted(line.split()[1] for line in text.splitlines() if line.startswith('#include'))
    assert includes == ['<cstddef>', '<cstdint>', '<new>', '<vector>'], includes


def test_layout_and_placement(tmp_path):
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.fail('g++ is needed to compile tests/csrc/stage_check.cpp')
    exe = str(tmp_path / 'stage_check')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', CSRC, SOURCE, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and 'stage_check ok' in r.stdout, (r.returncode, r.stdout + r.stderr)
