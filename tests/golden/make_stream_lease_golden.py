"""Generates tests/golden/ref_stream_lease_cfg5_ticks.npz: a leased stream at the registry of
BASELINE.json configs[4] (synth cfg5, 2000 servants) replayed for TICKS ticks through the VERBATIM
reference (oracle/_ref) by tests/stream_lease_model.run_reference: heartbeats as KeepServantAlive,
renewals as KeepTaskAlive, frees as FreeTask, OnExpirationTimer, reports as
NotifyServantRunningTasks, every batch as sequential WaitForStartingNewTask calls, leases of
now + {1, 2, 5, 40} ticks (seeded).
Stored per tick: digests of the answers, of the granted ids, of out_renewed, of out_report_unknown
and of running_tasks, |L| and the tick's counts. The run must contain expiries, sweeps, refused
renewals, unknown reported ids, ignored frees, Timeout answers and a zombie that survives because
its servant did not report (stream_lease_model.check_conditions). The GPU test
(tests/test_stream_lease_gpu.py) replays the same stream through ydc_stream_tick_leased and the CPU
test (tests/test_stream_lease_model.py) through the model. Needs the reference sources to build
oracle/_ref: python tests/golden/make_stream_lease_golden.py   (~4 min)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refbind as R  # noqa: E402
from tests import stream_lease_model as M  # noqa: E402
from yadcc_amd import synth  # noqa: E402

TICKS, TASKS, FREES, RENEWALS = 64, 9_000, 2_500, 800


def main():
    assert R.available(), "oracle/_ref is not built (needs the reference sources)"
    sv, _ = synth.make_config("cfg5")
    t0 = time.time()
    rec = M.run_reference(sv, TASKS, FREES, RENEWALS, TICKS)
    d = M.digests(rec)
    M.check_conditions(d)
    out = os.path.join(ROOT, "tests", "golden", "ref_stream_lease_cfg5_ticks.npz")
    np.savez_compressed(out, ticks=np.uint32(TICKS), tasks=np.uint32(TASKS), frees=np.uint32(FREES),
                        renewals=np.uint32(RENEWALS), **d)
    print("wrote %s: %d ticks in %.0f s; %s" % (out, TICKS, time.time() - t0,
                                                {k: int(d[k].sum()) for k in M.FIELDS[6:]}))
    print("max |L| %d" % int(d["n_leases"].max()))


if __name__ == "__main__":
    main()
