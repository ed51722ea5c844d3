#!/usr/bin/env python3
"""Record the SHA-256 digests tests/test_gpu_step_diet.py compares with:  step_diet_digests.py OUT.json

Run on an MI355X with the library of the commit whose bytes are to be pinned (CATINT_PNP_LIB names another build than the tree's).
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from tests import test_gpu_step_diet as T      # noqa: E402

with pytest.MonkeyPatch.context() as mp:
    out = T.all_digests(mp)
with open(sys.argv[1], 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print('%d cases written to %s' % (len(out), sys.argv[1]))
