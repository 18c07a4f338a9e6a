"""Writes tests/golden/ref_stream_rpc_cfg5_ticks.npz: what the VERBATIM reference class answered,
tick by tick, to the seeded cfg5 rpc stream of tests/stream_rpc_model.py (per-tick digests and
counts only). Needs oracle/_ref (make oracle). Run from the repository root:
    python -m tests.golden.make_stream_rpc_golden
"""
import os

import numpy as np

from tests import stream_rpc_model as M
from tests.test_stream_rpc_model import BIG

RPCS, FREES, RENEWALS, TICKS, MAX_WAITING, MAX_ROWS = 10, 200, 100, 72, 400, 16384


def main():
    sv = M.cfg5_one_slot()
    rec = M.run_reference(sv, RPCS, FREES, RENEWALS, TICKS, MAX_WAITING, MAX_ROWS, **BIG)
    d = M.digests(rec)
    M.check_conditions(d)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_stream_rpc_cfg5_ticks.npz")
    np.savez_compressed(out, rpcs=RPCS, frees=FREES, renewals=RENEWALS, ticks=TICKS, max_waiting=MAX_WAITING,
                        max_rows=MAX_ROWS, **d)
    print(out, os.path.getsize(out), "bytes; shares", M.shares(d))


if __name__ == "__main__":
    main()
