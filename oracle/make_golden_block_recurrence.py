#!/usr/bin/env python
"""TEST INFRASTRUCTURE: the scale vectors of the UNMODIFIED reference's `_layer_equalization` (dfq.py:29-75) on the
inverted-residual block of tests/test_closed_form_statistics.py, 30 sweeps, unsigned and signed
-> tests/golden/block_recurrence_ref.npz (s1_<kind>, s2_<kind>: float32 [sweeps, channels]).

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_block_recurrence.py

Needs oracle/_ref (the reference byte-compiled by oracle/build_ref.py, run by __graft_entry__.build()); with the stored
vectors test_block_recurrence_against_the_reference_itself runs where the reference is not present.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True

import test_closed_form_statistics as t      # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'block_recurrence_ref.npz')


def main():
    if not os.path.isfile(os.path.join(t.REFDIR, 'dfq.pyc')):
        raise SystemExit('oracle/_ref is not built (oracle/build_ref.py)')
    arrays = {}
    for signed, tag in ((False, 'unsigned'), (True, 'signed')):
        arrays['s1_' + tag], arrays['s2_' + tag] = t.reference_block_scales(signed)
    np.savez_compressed(OUT, **arrays)
    print('wrote {} ({})'.format(OUT, ', '.join('{} {}'.format(k, v.shape) for k, v in arrays.items())))


if __name__ == '__main__':
    main()
