"""Generates tests/golden/ref_stream_wait_lease_cfg5_ticks.npz: a waiting + leased stream at the
registry of BASELINE.json configs[4] (synth cfg5, 2000 servants) replayed for TICKS ticks through
the VERBATIM reference (oracle/_ref) by tests/stream_wait_lease_model.run_reference: heartbeats as
KeepServantAlive, renewals as KeepTaskAlive, frees as FreeTask, OnExpirationTimer, reports as
NotifyServantRunningTasks, every batch (the live queue, then the new requests) as sequential
WaitForStartingNewTask calls, each grant's lease set right behind it to now + lease_for with
lease_for in {1, 2, 5, 40} ticks and deadlines of now + {0, 1, 2, 5, 40} (seeded). The request
rate alternates (24 full ticks, 12 at an eighth), so the pool is saturated part of the time and
roomy part of the time.
Stored per tick: digests of the answers, of the new grants' ids, of the resolved list (tags,
answers, ids), of out_renewed, of out_report_unknown and of running_tasks, |W|, |L| and the tick's
counts. The run must contain what stream_wait_lease_model.check_conditions asks for: entries granted
from W, entries of W expired by deadline, requests that joined W, leases expired, swept, freed by
id, refused renewals, a tick with grants in both regions of the batch and a lease that was granted
from W and later became a zombie. The GPU test (tests/test_stream_wait_lease_gpu.py) replays the
same stream through ydc_stream_tick_waiting_leased and the CPU test
(tests/test_stream_wait_lease_model.py) through the model. Needs the reference sources to build
oracle/_ref: python tests/golden/make_stream_wait_lease_golden.py   (~5 min)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refbind as R  # noqa: E402
from tests import stream_wait_lease_model as M  # noqa: E402
from yadcc_amd import synth  # noqa: E402

TICKS, TASKS, FREES, RENEWALS, MAX_WAITING = 72, 9_000, 2_500, 800, 20_000


def main():
    assert R.available(), "oracle/_ref is not built (needs the reference sources)"
    sv, _ = synth.make_config("cfg5")
    t0 = time.time()
    rec = M.run_reference(sv, TASKS, FREES, RENEWALS, TICKS, MAX_WAITING)
    d = M.digests(rec)
    M.check_conditions(d)
    out = os.path.join(ROOT, "tests", "golden", "ref_stream_wait_lease_cfg5_ticks.npz")
    np.savez_compressed(out, ticks=np.uint32(TICKS), tasks=np.uint32(TASKS), frees=np.uint32(FREES),
                        renewals=np.uint32(RENEWALS), max_waiting=np.uint32(MAX_WAITING), **d)
    print("wrote %s: %d ticks in %.0f s; %s" % (out, TICKS, time.time() - t0,
                                                {k: int(d[k].sum()) for k in M.COUNTS}))
    print("max |W| %d, max |L| %d" % (int(d["n_waiting"].max()), int(d["n_leases"].max())))


if __name__ == "__main__":
    main()
