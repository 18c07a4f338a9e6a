"""The HOST class GpuTaskDispatcher without a GPU: gpu_task_dispatcher.cc + td_api.cc linked
against the CPU stand-in of the device API (tests/native/ydc_stub.cc over the CPU model of
tests/model) — locks, request combining, leases, digest / host interning, registry deltas and
servant expiry checked against the reference class itself on this box, plus the sanitizer
builds (`make -C tests/native tsan asan`). Placement arithmetic on the DEVICE
is what the -m gpu twin of this file (tests/test_task_dispatcher_gpu.py) checks; the product
library has no CPU placement."""
import ctypes as C
import os
import subprocess

import pytest

from oracle import refbind as R
from tests import td_scenarios as S
from yadcc_amd import dispatcher as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
_stub = None


class StubTaskDispatcher(D.GpuTaskDispatcher):
    @staticmethod
    def _load():
        global _stub
        if _stub is None:
            subprocess.check_call(["make", "-s", "-C", NATIVE, "all"])
            _stub = D.type_td_functions(C.CDLL(os.path.join(NATIVE, "libtd_stub.so")))
        return _stub


def make(**kw):
    d = StubTaskDispatcher(device=0, **kw)
    assert d.device_status == 0
    return d


@pytest.fixture
def td():
    d = make()
    yield d
    d.close()


def test_golden_all(td):
    S.golden_all(td)


def test_golden_prefer_dedicated(td):
    S.golden_prefer_dedicated(td)


def test_golden_load_balance(td):
    S.golden_load_balance(td)


def test_lease_table_churn():
    S.lease_table_churn(make)


def test_blocking_wait_is_woken_by_free_task():
    S.blocking_wait_is_woken_by_free_task(make)


def test_heartbeat_wakes_nobody():
    S.heartbeat_wakes_nobody(make)


def test_timer_tick_wakes_parked_waiters():
    S.timer_tick_wakes_parked_waiters(make)


def test_concurrent_callers_are_combined():
    S.concurrent_callers_are_combined(make)


def test_location_that_does_not_fit_is_an_error():
    S.location_that_does_not_fit_is_an_error(make)


def test_address_forms():
    S.address_forms(make)


@needs_ref
@pytest.mark.parametrize("seed", [5, 6])
def test_address_prefix_forms(seed):
    S.address_prefix_forms(make, seed)


@needs_ref
@pytest.mark.parametrize("seed", [1, 2])
def test_event_stream_matches_reference(seed):
    S.event_stream_matches_reference(make, seed)


@needs_ref
def test_event_stream_150_digests():
    dump = S.event_stream_matches_reference(make, 11, n_digests=150, n_pool=120, steps=500)
    assert dump["gpu"]["environment_mask_words"] >= 2


@pytest.mark.parametrize("san", ["tsan", "asan"])
def test_sanitizer_build(san):
    """ThreadSanitizer / AddressSanitizer + UBSan builds of the host class under concurrent
    callers (tests/native/td_concurrency_test.cc)."""
    out = subprocess.run(["make", "-s", "-C", NATIVE, san], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "TD-CONCURRENCY-OK" in out.stdout, (out.stdout[-2000:],
                                                                     out.stderr[-4000:])


ALIAS_TURN_CASES = "ABCD"


def _alias_turn(target, out_dir):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run(["make", "-s", "-C", NATIVE, target, "ALIASTURN_OUT=%s" % out_dir], capture_output=True,
                         text=True, timeout=600, env=env)
    assert out.returncode == 0 and "TD-ALIAS-TURN-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-6000:])


@pytest.fixture(scope="module")
def alias_turn_logs(tmp_path_factory):
    """What the ASan + UBSan build of tests/native/td_alias_turn_test.cc wrote for its cases."""
    out_dir = tmp_path_factory.mktemp("alias_turn")
    _alias_turn("aliasturn", out_dir)
    return out_dir


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_alias_turn_sanitized(san, alias_turn_logs, tmp_path):
    """One turn of UnsafeDrainQueue in which renumbering the parked waiters creates a requestor alias
    (a waiter parked from "[fe80", then "[fe80:1]:8335" registers) while new requests arrive — held
    together by a clock that blocks the registering thread under the dispatcher's lock
    (tests/native/td_alias_turn_test.cc). A: 24 arrivals of 24 triples against one parked triple — a
    turn that keeps the arrivals' numbers from before the renumbering reads sig_dead_ out of bounds
    (AddressSanitizer: heap-buffer-overflow in UnsafeDrainQueue); B: the stale number collides with
    the parked triple's and the arrival is answered Timeout unsent, where the reference grants it;
    C: two aliases in one turn; D: the alias's servant expires again under a parked waiter."""
    if san == "tsan":
        _alias_turn("aliasturn_tsan", tmp_path)
    for case in ALIAS_TURN_CASES:
        assert (alias_turn_logs / ("alias_turn_%s.json" % case)).exists()


@needs_ref
@pytest.mark.parametrize("case", list(ALIAS_TURN_CASES))
def test_alias_turn_matches_reference(case, alias_turn_logs):
    """... and each case's logged order, replayed through the reference class, gives the same answers
    and the same final DumpInternals; every thread finds its calls in program and real-time order."""
    import json
    j = json.load(open(alias_turn_logs / ("alias_turn_%s.json" % case)))
    threads = [{"ip": t["ip"], "ops": [(o[0], tuple(o[1:4]), o[4], o[5]) if o[0] == "wait" else (o[0], o[1], o[2], o[3])
                                       for o in t["ops"]]} for t in j["threads"]]
    n = S.verify_linearizable(j["log"], j["dump"], threads)
    waits = [e for e in j["log"] if e["op"] == "wait"]
    assert n >= 20 and any(e["ip"] == "[fe80" for e in waits)
    if case == "B":  # the request the unfixed turn declared a known Timeout
        assert [(e["st"], e.get("loc")) for e in waits if e["ip"] == "7.7.7.7"] == [(D.GRANTED, "[fe80:1]:8335")]


def test_flat_string_map_against_unordered_map():
    """The host class's string tables (yadcc_amd/csrc/flat_string_map.h: open addressing, backward
    shift on erase, miss filter) against std::unordered_map under random inserts / lookups /
    erases, ASan + UBSan build (tests/native/flat_map_test.cc)."""
    out = subprocess.run(["make", "-s", "-C", NATIVE, "flatmap"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "FLAT-MAP-OK" in out.stdout, (out.stdout[-2000:],
                                                                 out.stderr[-4000:])


@needs_ref
@pytest.mark.parametrize("seed", [1, 2])
def test_concurrent_callers_linearize(seed):
    """12 caller threads + a freer, a heartbeat thread and the clock / timer thread on 2000
    servants; the order in which their calls took effect, replayed one call at a time through the
    reference, gives the same answers and the same final state."""
    r = S.concurrent_callers_linearize(make, seed=seed)
    assert r["records"] > 5000 and r["kinds"].get("wait:0", 0) > 1000 and r["kinds"].get("timer", 0) > 3


@needs_ref
@pytest.mark.parametrize("shape", ["roomy", "saturated", "crowd", "prefixes"])
def test_native_callers_linearize(shape, tmp_path):
    """The same proof with the threads in C++ (tests/native/td_linearize.cc, through the C-ABI): 12
    callers at full speed, so that FreeTask queued behind somebody's device turn and the same
    thread's next request do meet in one turn (a build that applies queued frees after placing
    fails here on program order). roomy: nobody parks, frees are queued; saturated: most requests
    park and are retried at FreeTask's wake-ups. prefixes: bracketed multi-colon locations on a
    saturated pool, requestor addresses from every prefix of them, servants registering and expiring
    during the run — parked waiters turn into requestor aliases and are renumbered in turns that
    have arrivals to serve (alias_renumbered_turns; seed 3 with 16 threads x 600 calls on 40 servants
    gives 5 to 20 such turns on the stand-in, seeds 1-6 at half the calls 3 to 9)."""
    subprocess.check_call(["make", "-s", "-C", NATIVE, "linearize"])
    if shape == "prefixes":
        r = S.native_linearize(os.path.join(NATIVE, "td_linearize_stub"), str(tmp_path / "lin.json"), seed=3,
                               n_servants=40, n_threads=16, calls=600, cap=1, shape="prefixes")
        assert r["alias_renumbered_turns"] >= 1
        assert r["records"] > 10000 and r["retried_attempts"] > 3000 and r["kinds"]["wait:0"] > 500
        return
    args = {"roomy": dict(n_servants=300, calls=1500), "saturated": dict(n_servants=40, calls=3000, cap=1),
            # crowd: more parked requests than one device turn takes — placed again in segments, those
            # whose (digest, version, host) already came back Timeout in the turn not sent at all
            "crowd": dict(n_servants=40, n_threads=160, calls=200, cap=1)}[shape]
    r = S.native_linearize(os.path.join(NATIVE, "td_linearize_stub"), str(tmp_path / "lin.json"), seed=3, **args)
    assert r["records"] > 20000 and r["kinds"]["wait:0"] > (500 if shape == "crowd" else 3000)
    if shape != "roomy":
        assert r["retried_attempts"] > 5000 and r["kinds"]["wait:2"] > 10000


@needs_ref
def test_native_callers_linearize_tsan(tmp_path):
    """... and under ThreadSanitizer: no report, and the logged order still equals the reference's."""
    subprocess.check_call(["make", "-s", "-C", NATIVE, "linearize"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = S.native_linearize(os.path.join(NATIVE, "td_linearize_tsan"), str(tmp_path / "lin.json"), n_servants=60,
                           n_threads=8, calls=600, seed=4, env=env)
    assert r["records"] > 3000


@needs_ref
@pytest.mark.parametrize("san", ["tsan", "asan"])
def test_native_callers_linearize_prefixes_sanitized(san, tmp_path):
    """The prefixes shape under ThreadSanitizer and under ASan + UBSan: no report, the logged order
    equals the reference's, and the run did renumber parked waiters into aliases with arrivals in the
    turn (seed 4, 16 threads x 300 calls on 40 servants: 2 to 6 such turns in either build here). A
    long-lived dispatcher's sig_dead_ keeps the capacity of earlier turns, so a stale index mostly
    stays inside the allocation: the bounds proof is test_alias_turn_sanitized, this is the soak."""
    subprocess.check_call(["make", "-s", "-C", NATIVE, "linearize"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = S.native_linearize(os.path.join(NATIVE, "td_linearize_" + san), str(tmp_path / "lin.json"), n_servants=40,
                           n_threads=16, calls=300, cap=1, seed=4, env=env, shape="prefixes")
    assert r["alias_renumbered_turns"] >= 1
    assert r["records"] > 3000 and r["retried_attempts"] > 1000


@needs_ref
def test_event_stream_at_scale_small():
    """The scaled differential's event mix (bulk frees, batches of 1..256, structural heartbeats,
    expiries under thousands of live leases) on the stand-in, reduced: the host class's side of it."""
    r = S.event_stream_at_scale(make, seed=3, n_pool=300, prefill=5000, steps=2500)
    assert r["live_low_water"] >= 4500
