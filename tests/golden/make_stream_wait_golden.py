"""Generates tests/golden/ref_stream_wait_cfg5_60_ticks.npz: a waiting stream at the shape of
BASELINE.json configs[4] (synth cfg5 registry, 2000 servants; 10k requests per tick, max_waiting
20k) replayed for 60 ticks through the VERBATIM reference (oracle/_ref) by
tests/stream_wait_model.run_reference — heartbeats as KeepServantAlive, frees by grant id, every
tick's batch (the queue's live entries, then the new requests; entries whose deadline has passed
leave as Timeout untried) as sequential WaitForStartingNewTask calls, the queue kept from the
reference's own answers. Deadlines are now + {0, 1, 2, 5, 40} ticks (seeded). 6k frees per tick
instead of cfg5's 10k: at 10k every live grant is freed each tick and nothing ever waits; at 6k the
pool saturates from tick 25 on and the queue holds up to ~9k requests.
Stored per tick: digests of the new requests' answers, of the resolved list (tags and answers),
its length, n_waiting and a digest of running_tasks. The GPU test
(tests/test_stream_waiting_gpu.py) replays the same stream through ydc_stream_tick_waiting and the
CPU test (tests/test_stream_wait_model.py) through the model. Run in the build container (needs
/root/reference): python tests/golden/make_stream_wait_golden.py   (~1 min)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refbind as R  # noqa: E402
from tests import stream_wait_model as M  # noqa: E402
from yadcc_amd import synth  # noqa: E402

TICKS, TASKS, FREES, MAX_WAITING = 60, 10_000, 6_000, 20_000


def main():
    assert R.available(), "oracle/_ref is not built (needs /root/reference)"
    sv, _ = synth.make_config("cfg5")
    t0 = time.time()
    rec = M.run_reference(sv, TASKS, FREES, TICKS, MAX_WAITING)
    d = M.digests(rec)
    out = os.path.join(ROOT, "tests", "golden", "ref_stream_wait_cfg5_60_ticks.npz")
    np.savez_compressed(out, ticks=np.uint32(TICKS), tasks=np.uint32(TASKS), frees=np.uint32(FREES),
                        max_waiting=np.uint32(MAX_WAITING), **d)
    print("wrote %s: %d ticks in %.0f s, max queue %d" % (out, TICKS, time.time() - t0, int(d["n_waiting"].max())))


if __name__ == "__main__":
    main()
