"""The dependency lists of catint_amd/build.py against the sources: every file a library's sources reach through quoted #include lines
(transitively, the public headers under include/ too) is one of its sources or in its header list.  A header missing from a list
leaves a stale library behind when only that header changes."""
import os
import re

import pytest

from catint_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)

LIBRARIES = {
    'pnp': (build.CSRC, build.SOURCES, build.HEADERS),
    'observe': (build.OBSERVE_DIR, build.OBSERVE_SOURCES, build.OBSERVE_HEADERS),
    'balance': (build.BALANCE_DIR, build.BALANCE_SOURCES, build.BALANCE_HEADERS),
    'unittest': (build.UNITTEST_DIR, build.UNITTEST_SOURCES, build.UNITTEST_HEADERS),
}


def reached(paths):
    seen, todo = set(), [os.path.realpath(p) for p in paths]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        with open(path) as f:
            for name in INCLUDE.findall(f.read()):
                inc = os.path.realpath(os.path.join(os.path.dirname(path), name))
                assert os.path.exists(inc), '%s includes %s, which does not exist' % (path, name)
                todo.append(inc)
    return seen


@pytest.mark.parametrize('name', sorted(LIBRARIES))
def test_every_included_file_is_a_listed_dependency(name):
    src_dir, sources, headers = LIBRARIES[name]
    sources = [os.path.join(src_dir, s) for s in sources]
    listed = {os.path.realpath(p) for p in sources + headers}
    assert len(listed) == len(sources + headers), 'a file is listed twice'
    found = reached(sources)
    assert os.path.realpath(os.path.join(build.CSRC, '..', '..', 'include', 'catint_pnp.h')) in found, 'the walk did not reach include/'
    missing = found - listed
    assert not missing, 'included but not in the dependency list of build.py: %s' % sorted(missing)
