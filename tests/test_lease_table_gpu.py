"""The device's lease table beyond a displacement of 1: chains of ids that share a home slot, holes
inside a chain, chains across the wrap from the last slot to slot 0, inserts that contend for the slots
behind a run, and the bound on the probe length (LeaseState::max_disp) through every kernel that keeps
it: the tick's insert, the rehash of ydc_stream_reserve, the load of ydc_stream_restore and the two
delta applies, each with and without inspection records.

Every context is opened by ydc_stream_restore of a blob that snapshot.build makes from the model's state
(tests/lease_table_cases.py: crafted_stream; no C writer involved), whose table holds ids computed to
collide. Every tick is one of that file's scripts, compared with tests/stream_lease_model.py through
check_tick (every output, running_tasks, the tick's counts, ydc_stream_leases_get); after each script
the C-written snapshot must parse to the model's state. tests/test_lease_table_model.py plays the same
scripts through the model alone and asserts the conditions the cases rest on.

  1 found_at_every_displacement   renewals and a report at every displacement, a non-member of the home
  2 holes_inside_the_chain        no tombstones: lookups walk past emptied slots ...
  3   (the same script)           ... which a burst of grants takes again
  4 contended_inserts             200 grants, >= 20 of them into the run, with and without inspection
  5 expiry_and_sweep              zombies on a chain, swept by their servants' reports
  6 reserve_with_a_chain          k_lease_rehash / k_inspect_rehash: the bound of the NEW table
  7 snapshot_and_restore          k_lease_load puts 257 threads on one home
  8 delta_to_a_standby            k_lease_delta_check / _apply_old / _apply_new / _apply_inspect, k_inspect_gather
  9 remove_servants_with_a_chain  k_lease_remap empties slots in the middle of a chain

No case intends an access outside the table or a probe without end: every probe loop of the library is
bounded by cap, and every table here is at most half full."""
import numpy as np
import pytest

from tests import lease_table_cases as C
from tests import stream_inspect_model as IM
from tests import stream_lease_model as M
from tests import stream_snapshot_model as SM
from tests.test_stream_inspect_delta_gpu import same_inspection
from tests.test_stream_lease_edges_gpu import Hand
from tests.test_stream_lease_gpu import check_tick, gpu_tick
from yadcc_amd import binding, snapshot

pytestmark = pytest.mark.gpu
SNAP = ("ids", "servants", "expires_at", "zombie")


def restored(blob):
    ctx = binding.Context(device=0)
    ctx.stream_restore(blob)
    return ctx


class Device(C.ModelDriver, Hand):
    """The scripts on restored contexts: every tick through the model, then on every context that is
    ticking (Hand's tick for one, the same comparison for each of two)."""

    def __init__(self, ls, caps, inspect=False):
        C.ModelDriver.__init__(self, ls, caps)
        self.blob = snapshot.build(C.state(ls, caps))
        self.ctx = restored(self.blob)
        assert self.ctx.stream_caps() == dict(caps, max_rows=0, max_waiting=0)
        assert self.ctx.stream_snapshot() == self.blob, "the C writer and snapshot.build disagree"
        self.all = self.live = [self.ctx]
        self.I = self.prev = None
        if inspect:
            self.I = IM.attach(ls)
            self.ctx.stream_inspect_begin(discovered_at=np.zeros(ls.es.n, np.int64))
            ids = sorted(self.T.L)
            k = np.arange(len(ids))
            rec = dict(task_id=np.array(ids, np.uint64), started_at=(100 + k).astype(np.int64), env_id=np.zeros(len(ids), np.uint32),
                       requestor_ip=(0x0C000000 + k).astype(np.uint32), prefetch=(k & 1).astype(np.uint8))
            self.ctx.stream_inspect_load(**rec)  # (k_inspect_find: every member by lookup)
            self.I.load(rec)
            self.inspected("after the load")

    def inspected(self, what):
        if self.I is not None:
            same_inspection(what, self.I, *self.live)

    def play(self, ev):
        if self.I is not None:
            self.T.inspect.stage(ev)
        if len(self.live) == 1:
            self.ctx, t = self.live[0], self.t
            want = Hand.tick(self, ev)
            self.t = t  # (ModelDriver.tick counts)
        else:
            want = M.model_tick(self.ls, ev)
            got = [gpu_tick(c, self.ls, ev) for c in self.live]
            for c, g in zip(self.live, got):
                check_tick(self.t, c, self.ls, g, want)
            for x, y in zip(*got):
                assert np.array_equal(x, y), "tick %d: outputs differ between the twins" % self.t
            assert self.live[0].stream_snapshot() == self.live[1].stream_snapshot(), "tick %d: the twins' snapshots differ" % self.t
        self.inspected("tick %d" % self.t)
        return want

    def twin(self, blob):
        b = restored(blob)
        assert b.stream_snapshot() == blob, "snapshot, restore, snapshot changed the bytes"
        if self.I is not None:
            b.stream_inspect_restore(self.ctx.stream_delta_inspect())
        self.all = [self.ctx, b]
        return b

    def reserve(self, max_leases):
        before = self.ctx.stream_leases()
        C.ModelDriver.reserve(self, max_leases)
        assert self.ctx.stream_reserve(max_leases=max_leases)["max_leases"] == max_leases
        for name, x, y in zip(SNAP, before, self.ctx.stream_leases()):
            assert np.array_equal(x, y), "the reserve changed the lease snapshot's %s" % name
        self.inspected("after the reserve")

    def remove(self, removed):
        self.ctx.remove_servants(np.asarray(removed, np.uint32))
        C.ModelDriver.remove(self, removed)
        for name, x, y in zip(SNAP, self.ctx.stream_leases(), self.T.snapshot()):
            assert np.array_equal(x, y), "after ydc_remove_servants: %s differs" % name
        assert np.array_equal(self.ctx.get_running(), self.ls.es.running.astype(np.uint32))

    def fork(self):
        blob = self.ctx.stream_snapshot()
        self.live = [self.ctx, self.twin(blob)]

    def base(self):
        blob = self.ctx.stream_delta_base()
        assert blob == self.ctx.stream_snapshot()
        self.standby, self.prev = self.twin(blob), snapshot.parse(blob)

    def take(self):
        """-> (the delta just taken on the primary, its sidecar or None, the primary's snapshot)."""
        delta = self.ctx.stream_delta()
        side = self.ctx.stream_delta_inspect(delta) if self.I is not None else None
        full = self.ctx.stream_snapshot()
        now = snapshot.parse(full)
        assert delta == snapshot.build_delta(self.prev, now), "the delta is not f(before, after)"
        self.prev = now
        return delta, side, full

    def apply(self, ctx, delta, side):
        if side is None:
            ctx.stream_delta_apply(delta)
        else:
            ctx.stream_delta_apply_inspected(delta, side)

    def delta(self):
        delta, side, full = self.take()
        self.apply(self.standby, delta, side)
        assert self.standby.stream_snapshot() == full, "the standby's snapshot is not the primary's"
        if self.I is not None:
            same_inspection("after the delta", self.I, self.ctx, self.standby)

    def only(self, who):
        assert who == "standby"
        self.live = [self.standby]

    def finish(self):
        """Every ticking context's snapshot is the model's state; everything is closed."""
        for c in self.live:
            SM.same(snapshot.parse(c.stream_snapshot()), C.state(self.ls, c.stream_caps(), self.t))
        if self.prev is not None:
            self.all[0].stream_delta_stop()
        for c in self.all:
            c.stream_end()
            c.close()


def run(script, make, case, inspect=False):
    ls, caps = C.crafted_stream(make(case))
    d = Device(ls, caps, inspect)
    script(d, case)
    d.finish()
    return d


def shapes(cases):
    return pytest.mark.parametrize("case", cases, ids=[c.name for c in cases])


@shapes(C.SHAPES)
def test_found_at_every_displacement_across_the_wrap(case):
    run(C.found_at_every_displacement, C.entries, case)


@shapes(C.SHAPES)
def test_no_tombstones_and_holes_are_taken_again(case):
    run(C.holes_inside_the_chain, C.entries, case)


@pytest.mark.parametrize("inspect", [False, True], ids=["plain", "inspected"])
@shapes(C.LONG)
def test_inserts_that_contend_for_the_slots_behind_a_run(case, inspect):
    """With inspection (lease_insert_inspected) each of the 200 has its own requestor, the members keep
    the records loaded for them: a record sits in the slot its thread won, not the one it first tried."""
    d = run(C.contended_inserts, C.entries, case, inspect)
    if inspect:
        assert len(set(d.I.tasks()["requestor_ip"].tolist())) == case.n + C.GRANTS // 2


@shapes(C.SHAPES)
def test_expiry_and_sweep_on_a_chain(case):
    run(C.expiry_and_sweep, C.expiry_entries, case)


@pytest.mark.parametrize("inspect", [False, True], ids=["k_lease_rehash", "k_inspect_rehash"])
@shapes([C.WHOLE_2048, C.SPLIT_2048])
def test_reserve_files_a_chain_again(case, inspect):
    """A chain that stays whole in the larger table is found only with the bound of the new table."""
    d = run(C.reserve_with_a_chain, C.entries, case, inspect)
    assert d.caps["max_leases"] == 1024


@shapes([C.BY_NAME["wrap3_257"], C.TOUCHING])
def test_snapshot_and_restore_of_a_chain(case):
    run(C.snapshot_and_restore, C.entries, case)


@pytest.mark.parametrize("inspect", [False, True], ids=["plain", "inspected"])
@shapes([C.BY_NAME["wrap3_257"], C.TOUCHING, C.TOUCHING_MID])
def test_delta_to_a_standby(case, inspect):
    run(C.delta_to_a_standby, C.delta_entries, case, inspect)


def test_a_delta_that_erases_what_the_standby_lacks_is_refused():
    """Two crafted blobs of one identity (tick number, next_id, |L|, clock, structure): the standby's holds
    another id of the same home in place of one member. The primary frees that member; the delta's
    header fits the standby, only k_lease_delta_check, which has to walk the chain, can tell. The
    standby stays as it was and answers a tick. (The check's other half, an inserted id that is a lease
    already, cannot be reached through the API: inserted ids are >= the base's next_id and a table
    holds only ids below its own.)"""
    case = C.BY_NAME["wrap3_257"]
    ls, caps = C.crafted_stream(C.entries(case))
    d = Device(ls, caps)
    d.prev = snapshot.parse(d.ctx.stream_delta_base())
    missing = case.ids[200]
    other = [(case.spare if t == missing else t, s, e, z) for t, s, e, z in C.entries(case)]
    ls2, caps2 = C.crafted_stream(other)
    d2 = Device(ls2, caps2)
    r = d.tick(free=[missing], n=8, lease=[C.FAR] * 8)
    assert r["freed"] == 1
    delta, _, _ = d.take()
    before = d2.ctx.stream_snapshot()
    with pytest.raises(binding.YdcError, match="invalid argument"):
        d2.ctx.stream_delta_apply(delta)
    assert d2.ctx.stream_snapshot() == before, "the refused delta changed the standby"
    r = d2.tick(renew=[(t, 5) for t in C.scrambled(sorted(d2.T.L))] + [(missing, 5)])
    assert r["renew_refused"] == 1 and int(r["renewed"].sum()) == case.n
    # ... and the standby that does hold it takes the same delta.
    d3 = restored(d.blob)
    d3.stream_delta_apply(delta)
    assert d3.stream_snapshot() == d.ctx.stream_snapshot()
    d3.stream_end()
    d3.close()
    d.finish()
    d2.finish()


@shapes([C.BY_NAME["wrap3_257"], C.TOUCHING_MID])
def test_remove_servants_with_a_chain_open(case):
    run(C.remove_servants_with_a_chain, C.entries, case)
