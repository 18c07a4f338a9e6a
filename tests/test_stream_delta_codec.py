"""The byte format of ydc_stream_delta / ydc_stream_delta_apply without a GPU.

State pairs come from the stream models (tests/stream_lease_model.py, stream_wait_lease_model.py,
stream_rpc_model.py with stream_book_model.py and stream_alive_model.py) through
tests/stream_snapshot_model.py: a model runs some ticks, its state is A; it runs on, its state is B.
For every pair yadcc_amd/snapshot.py's build(apply_delta(A, build_delta(A, B))) must equal build(B) byte
for byte, and the C++ build of yadcc_amd/csrc/stream_delta_codec.h (tests/native/delta_codec_test.cc,
ASan + UBSan, given the two snapshots as files) must give the very bytes numpy's build_delta gives.
parse_delta refuses every kind of bad blob the C validator names, and the C validator runs over good
blobs and seeded corruptions as a program of its own. Every test fails without the feature:
snapshot.py has no build_delta and the codec header does not exist."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import stream_alive_model as AM
from tests import stream_book_model as BM
from tests import stream_lease_model as L
from tests import stream_rpc_cases as rcases
from tests import stream_rpc_model as RM
from tests import stream_snapshot_model as SM
from tests import stream_wait_lease_cases as wcases
from tests import stream_wait_lease_model as WM
from tests.conftest import ROOT
from yadcc_amd import snapshot as S, synth

LEASE_CAPS = dict(max_updates=16, max_releases=16, max_tasks=64, max_leases=4096, max_renewals=4096, max_frees=4096,
                  max_reports=64, max_report_ids=4096)
FAR = 1 << 40


def pool(n=8, slots=64):
    sv = synth.make_servants(n, n_tasks_hint=n * slots, n_envs=1, seed=42)
    sv["num_processors"][:], sv["current_load"][:] = 4096, 0
    sv["max_tasks"][:], sv["running_tasks"][:] = slots, 0
    return sv


class Leased:
    """The lease model with hand-made traffic; parsed() is the state as a parsed full snapshot."""

    def __init__(self, first_id=0):
        self.ls = L.LeaseStream(pool(), 0, 0, 0, L.LeaseTable(), n_envs=1)
        self.ls.es.hb = 2
        self.ls.table.next_id = first_id
        self.t = 0

    def tick(self, n=0, expires_at=FAR, **over):
        ev = dict(self.ls.next_tick())
        none64 = np.empty(0, np.uint64)
        ev.update(renew_ids=none64, renew_expires_at=np.empty(0, np.int64), free_ids=none64,
                  report_servants=np.empty(0, np.uint32), report_off=np.zeros(1, np.uint32), report_ids=none64,
                  tasks=synth.make_tasks(n, self.ls.es.sv, n_envs=1, seed=self.t + 1, self_frac=0.0), release_idx=np.empty(0, np.uint32),
                  lease_expires_at=np.broadcast_to(np.asarray(expires_at, np.int64), (n,)).copy())
        ev.update(over)
        self.t += 1
        return L.model_tick(self.ls, ev)

    def ids(self):
        return np.array(sorted(self.ls.table.L), np.uint64)

    def parsed(self):
        return S.parse(S.build(SM.state_of("leased", self.ls, LEASE_CAPS, self.t)))


def report(lists):
    off = np.cumsum([0] + [len(ids) for _, ids in lists]).astype(np.uint32)
    return dict(report_servants=np.array([s for s, _ in lists], np.uint32), report_off=off,
                report_ids=np.array([t for _, ids in lists for t in ids], np.uint64))


def stamped(p, ids, stamp):
    """The parsed state with the report stamp of the leases `ids` set (the models keep none)."""
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    hit = np.isin(q["l_id"], np.asarray(ids, np.uint64))
    q["l_state"][hit] = (q["l_state"][hit] & ~np.uint32(S.STAMP)) | np.uint32(stamp)
    return S.parse(S.build({k: v for k, v in q.items() if k not in ("l_zombie", "l_stamp")}))


def leased_pairs():
    out = {}
    m = Leased()
    m.tick(40)
    a = m.parsed()
    out["no change"] = (a, a, dict(n_ins=0, n_era=0, n_upd=0))
    m.tick(25)
    b = m.parsed()
    out["only inserts"] = (a, b, dict(n_ins=25, n_era=0, n_upd=0))
    m.tick(0, free_ids=m.ids()[5:30])
    c = m.parsed()
    out["only erases"] = (b, c, dict(n_ins=0, n_era=25, n_upd=0))
    m.tick(0, renew_ids=m.ids(), renew_expires_at=np.full(len(m.ids()), FAR + 9, np.int64))
    d = m.parsed()
    out["renewals only"] = (c, d, dict(n_ins=0, n_era=0, n_upd=40))
    out["over several ticks"] = (a, d, dict(n_ins=25, n_era=25, n_upd=15))  # (ids 5 .. 29 freed, 40 .. 64 new, the other 15 renewed)
    m.tick(0, free_ids=m.ids())
    e = m.parsed()
    out["all of L erased"] = (d, e, dict(n_ins=0, n_era=40, n_upd=0, n_leases=0))
    m.tick(1)
    f = m.parsed()
    out["|L| 0 -> 1"] = (e, f, dict(n_ins=1, n_era=0, n_upd=0, base_n_leases=0))
    m.tick(1, free_ids=m.ids())
    out["|L| 1 -> 1, another lease"] = (f, m.parsed(), dict(n_ins=1, n_era=1, n_upd=0))
    # Expiry to zombie, then a stamp.
    z = Leased()
    z.tick(30, expires_at=np.where(np.arange(30) < 10, 1, FAR))
    a = z.parsed()
    want = z.tick(0)
    want = want if want["expired"] else z.tick(0)
    assert want["expired"] == 10
    b = z.parsed()
    assert b["l_zombie"].sum() == 10
    out["a zombie bit set"] = (a, b, dict(n_ins=0, n_era=0, n_upd=10))
    out["a stamp set"] = (b, stamped(b, z.ids()[3:7], z.t), dict(n_ins=0, n_era=0, n_upd=4))
    # Ids from 2^40.
    h = Leased(first_id=1 << 40)
    h.tick(20)
    a = h.parsed()
    h.tick(20, free_ids=h.ids()[::2])
    b = h.parsed()
    assert int(b["l_id"].min()) > 1 << 40
    out["ids from 2^40"] = (a, b, dict(n_ins=20, n_era=10, n_upd=0))
    return out


def wait_leased_pairs():
    sv = wcases.small_stream().es.sv
    ws = WM.new_stream(sv, 48, 0, 0, 64, n_envs=1, rate=lambda now: 1.0)
    ws.es.hb = ws.es.n
    caps = dict(LEASE_CAPS, max_waiting=64)
    t = [0]

    def tick(**kw):
        t[0] += 1
        return WM.model_tick(ws, wcases.scripted(ws, ws.next_tick(), **kw))

    def parsed():
        return S.parse(S.build(SM.state_of("wait_leased", ws, caps, t[0])))

    k = np.arange(48)
    assert tick(n=48, lease_for=20 + 3 * k, wait=2 + k % 5)["n_waiting"] >= 8
    a = parsed()
    tick(n=5, lease_for=9, wait=2, free=sorted(ws.state.T.L)[:6])
    b = parsed()
    assert len(a["w_tag"]) != len(b["w_tag"]) or not np.array_equal(a["w_tag"], b["w_tag"])
    return {"waiting and leased": (a, b, dict(n_era=6))}


def rpc_pairs():
    out = {}
    ws = rcases.small_stream(max_rows=3000, max_waiting=64)
    caps = dict(LEASE_CAPS, max_tasks=24, max_rows=3000, max_waiting=64)
    shapes = [(1, 2), (3, 0), (0, 2), (2, 3), (1, 0), (4, 1), (0, 1)]
    RM.model_tick(ws, rcases.scripted(ws, ws.next_tick(), rpcs=[(200, 100, 30, 5)] + [(a, b, 10 + a, 20 + b) for a, b in shapes]))
    a = S.parse(S.build(SM.state_of("rpc", ws, caps, 1)))
    RM.model_tick(ws, rcases.scripted(ws, ws.next_tick(), rpcs=[(1, 1, 7, 15)] * 3, free=sorted(ws.state.T.L)[:4]))
    b = S.parse(S.build(SM.state_of("rpc", ws, caps, 2)))
    assert a["n_wait_rows"] > 0 and b["n_wait_rows"] > 0 and a["rpc"]
    out["rpc rows, B off, E off"] = (a, b, dict(book_present=0))
    # With the book and aliveness (no servant expires: that would be another structure).
    from tests import test_stream_alive_gpu as alive
    sv = synth.make_servants(70, n_tasks_hint=2400, n_envs=2, seed=3)
    ws = RM.new_stream(sv, 40, 300, 100, 1000, 1 << 12, n_envs=2, report_frac=0.3, **alive.BIG)
    ws.es.hb = alive.HB
    book = BM.Book(6000)
    A = AM.attach(ws, np.full(70, FAR, np.int64), book)
    gen = AM.AliveGen(ws, life=FAR, p_stop=0, p_short=0)
    caps = dict(LEASE_CAPS, max_updates=alive.HB + 8, max_tasks=40, max_rows=1 << 12, max_waiting=1000, max_leases=1 << 14,
                max_reports=70, max_report_ids=1 << 14)
    t = [0]

    def tick():
        ev = gen.next_tick()
        book.stage(*BM.payload(ev))
        t[0] += 1
        return AM.model_tick(RM, ws, ev)

    def parsed():
        return S.parse(S.build(SM.state_of("rpc", ws, caps, t[0], book, A, 6000)))

    for _ in range(4):
        tick()
    a = parsed()
    for _ in range(3):
        tick()
    b = parsed()
    assert len(b["b_grant_id"]) > 0 and ws.es.n == 70 and b["alive"] and b["book"]
    assert not np.array_equal(a["e_expires_at"], b["e_expires_at"]), "no heartbeat moved E"
    out["rpc, B changed, E on"] = (a, b, dict(book_present=1))
    out["rpc, B unchanged, E on"] = (b, b, dict(book_present=0, n_ins=0, n_era=0, n_upd=0))
    return out


def all_pairs():
    if not hasattr(all_pairs, "made"):
        all_pairs.made = dict(leased_pairs(), **wait_leased_pairs(), **rpc_pairs())
    return all_pairs.made


PAIR_NAMES = ["no change", "only inserts", "only erases", "renewals only", "over several ticks", "all of L erased", "|L| 0 -> 1",
              "|L| 1 -> 1, another lease", "a zombie bit set", "a stamp set", "ids from 2^40", "waiting and leased",
              "rpc rows, B off, E off", "rpc, B changed, E on", "rpc, B unchanged, E on"]


def test_the_pairs_are_all_listed():
    assert sorted(all_pairs()) == sorted(PAIR_NAMES)


@pytest.mark.parametrize("name", PAIR_NAMES)
def test_apply_of_build_is_the_later_state(name):
    a, b, want = all_pairs()[name]
    delta = S.build_delta(a, b)
    d = S.parse_delta(delta)
    for k, v in want.items():
        assert d[k] == v, (k, d[k], v)
    assert d["stamp"] == S.structure_stamp(a) == S.structure_stamp(b)
    assert (d["base_next_id"], d["base_lease_tick"], d["base_last_now"]) == (a["next_id"], a["lease_tick"], a["last_now"])
    got = S.apply_delta(a, delta)
    assert S.build(got) == S.build(b), "build(apply_delta(A, build_delta(A, B))) is not build(B)"
    assert S.build_delta(a, got) == delta, "the delta is not a function of the two states alone"
    # What the issue expects a delta to weigh: the lists, the light columns, W, E, and B only when it changed.
    n, n_w = len(b["version"]), len(b["w_tag"]) if b["waiting"] else 0
    w_width = 36 + (8 if b["rpc"] else 0)
    pad = S._pad8
    assert len(delta) == 272 + 24 * d["n_ins"] + 8 * d["n_era"] + pad(20 * d["n_upd"]) + pad(28 * n) + pad(w_width * n_w) + (
        8 * n if b["alive"] else 0) + (pad(28 * d["n_book"]) if d["book_present"] else 0)
    if a is not b and name != "a stamp set":
        with pytest.raises(S.FormatError):  # (applied, the delta's base is gone: twice is refused)
            S.apply_delta(got, delta)


def test_build_delta_refuses_what_a_delta_does_not_carry():
    a, b, _ = all_pairs()["only inserts"]
    for change in (dict(max_leases=8192), dict(ip_id=b["ip_id"] + np.uint32(1)), dict(alias_ip=np.array([5], np.uint32),
                                                                                     alias_servant=np.array([1], np.uint32)),
                   dict(env_mask=b["env_mask"] ^ np.uint64(2))):
        other = S.parse(S.build({k: v for k, v in dict(b, **change).items()}))
        with pytest.raises(S.FormatError, match="structure"):
            S.build_delta(a, other)
    moved = dict(b, l_servant=(b["l_servant"] + np.uint32(1)) % np.uint32(len(b["version"])))
    with pytest.raises(S.FormatError, match="servant"):
        S.build_delta(a, S.parse(S.build(moved)))
    with pytest.raises(S.FormatError):  # (backwards: freed ids would appear below the base's next_id)
        S.build_delta(*all_pairs()["only erases"][1::-1])


def sealed(b):
    b = bytearray(b)
    b[24:32] = S.checksum(bytes(b)).to_bytes(8, "little")
    return bytes(b)


def test_parse_delta_refuses_corruptions():
    a, b, _ = all_pairs()["rpc, B changed, E on"]
    blob = S.build_delta(a, b)
    head = S.DELTA_HEADER.unpack_from(blob)
    d = S.parse_delta(blob)
    off = {name: head[31 + 2 * k] for k, name in enumerate(S.DELTA_SECTIONS)}
    n_ins, n_era, n_upd, n = d["n_ins"], d["n_era"], d["n_upd"], d["n_servants"]
    assert min(n_ins, n_era, n_upd) >= 2 and d["n_waiting"] >= 1 and d["n_book"] >= 1
    F = {name: 32 + 4 * k for k, name in enumerate(("mode", "env_words", "n_servants", "book_present", "max_leases",
                                                    "max_waiting", "max_rows", "max_book"))}
    F.update(base_next_id=72, base_last_now=80, base_lease_tick=88, base_n_leases=92, base_n_waiting=96, reserved=100,
             next_id=104, last_now=112, alive_bound=120, lease_tick=128, n_leases=132, n_waiting=136, n_wait_rows=140,
             n_book=144, n_ins=148, n_era=152, n_upd=156, dir=160)
    for k, at in F.items():  # (the offsets above are the header's)
        if k != "dir":
            width = 8 if k in ("base_next_id", "base_last_now", "next_id", "last_now", "alive_bound") else 4
            assert int.from_bytes(blob[at:at + width], "little", signed=k.endswith(("now", "bound"))) == d[k], k

    def put(at, value, width=4):
        out = bytearray(blob)
        out[at:at + width] = (int(value) % (1 << (8 * width))).to_bytes(width, "little")
        return sealed(out)

    def u64(at):
        return int.from_bytes(blob[at:at + 8], "little")

    w_npre = off["W"] + d["n_waiting"] * 40
    bad = {
        "cut at the header": blob[:100],
        "cut inside a section": blob[:off["registry"] + 20],
        "one byte short": blob[:-1],
        "eight bytes short": blob[:-8],
        "a byte behind": blob + b"\0",
        "eight zero bytes behind, sealed": sealed(blob + bytes(8)),
        "flipped byte in the header": blob[:41] + bytes([blob[41] ^ 1]) + blob[42:],
        "flipped byte in the inserts": blob[:off["inserted"] + 5] + bytes([blob[off["inserted"] + 5] ^ 0x80]) + blob[off["inserted"] + 6:],
        "not a delta": put(0, S.MAGIC, 8),
        "unknown version": put(8, 2),
        "header size": put(12, 280),
        "unknown mode bit": put(F["mode"], d["mode"] | 32),
        "mode without L": put(F["mode"], d["mode"] & ~2),
        "mode without the book": put(F["mode"], d["mode"] & ~8),
        "env_words 0": put(F["env_words"], 0),
        "book_present 2": put(F["book_present"], 2),
        "reserved set": put(F["reserved"], 1),
        "max_waiting 0": put(F["max_waiting"], 0),
        "|L| beyond max_leases": put(F["max_leases"], d["n_leases"] - 1),
        "n_servants + 1": put(F["n_servants"], n + 1),
        "n_ins + 1": put(F["n_ins"], n_ins + 1),
        "n_era 2^32 - 1": put(F["n_era"], 0xFFFFFFFF),
        "|L| off by one": put(F["n_leases"], d["n_leases"] + 1),
        "next_id below the base's": put(F["next_id"], d["base_next_id"] - 1, 8),
        "the clock runs backwards": put(F["last_now"], d["base_last_now"] - 1, 8),
        "a tick number whose stamp is 0": put(F["lease_tick"], 1 << 30),
        "rows(W) off by one": put(F["n_wait_rows"], d["n_wait_rows"] + 1),
        "section offset moved": put(F["dir"] + 16, off["erased"] + 8, 8),
        "section size 2^63": put(F["dir"] + 24, 1 << 63, 8),
        "inserted ids not ascending": put(off["inserted"] + 8, u64(off["inserted"]), 8),
        "inserted id below the base's next_id": put(off["inserted"], d["base_next_id"] - 1, 8),
        "inserted id == next_id": put(off["inserted"] + 8 * (n_ins - 1), d["next_id"], 8),
        "inserted servant == n_servants": put(off["inserted"] + 16 * n_ins, n),
        "inserted lease without the live bit": put(off["inserted"] + 20 * n_ins, 7),
        "erased ids not ascending": put(off["erased"], u64(off["erased"] + 8) + 1, 8),
        "erased id >= the base's next_id": put(off["erased"] + 8 * (n_era - 1), d["base_next_id"], 8),
        "updated ids not ascending": put(off["updated"] + 8, u64(off["updated"]), 8),
        "updated id 2^64 - 1": put(off["updated"] + 8 * (n_upd - 1), (1 << 64) - 1, 8),
        "updated lease without the live bit": put(off["updated"] + 16 * n_upd, 1 << 30),
        "a lease erased and updated": put(off["updated"], max(int(x) for x in d["era_id"] if x < d["upd_id"][1]), 8)
        if (d["era_id"] < d["upd_id"][1]).any() else put(off["erased"], int(d["upd_id"][0]), 8),
        "an RPC of no rows": sealed(bytearray(put(w_npre - 4 * d["n_waiting"], 0))[:w_npre] + bytes(4) + bytearray(put(w_npre - 4 * d["n_waiting"], 0))[w_npre + 4:]),
        "E below alive_bound": put(off["E"], d["alive_bound"] - 1, 8),
        "book entry on no servant": put(off["B"] + 24 * d["n_book"], n),
    }
    pad_at = next((off[s] + used for s, used in (("updated", 20 * n_upd), ("registry", 28 * n), ("B", 28 * d["n_book"]))
                   if used % 8), None)
    assert pad_at is not None, "no section of this delta has padding"
    bad["padding not zero"] = put(pad_at, 1, 1)
    for name, bytes_ in bad.items():
        with pytest.raises(S.FormatError):
            S.parse_delta(bytes_)
            pytest.fail("%s was accepted" % name)
    assert S.parse_delta(sealed(blob))["n_ins"] == n_ins


@pytest.fixture(scope="module")
def codec_tool(tmp_path_factory):
    """tests/native/delta_codec_test.cc: includes only the two codec headers; ASan + UBSan, built the way
    test_stream_snapshot_codec.py builds its twin, and run as a program of its own."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("delta_codec") / "delta_codec_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "delta_codec_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_c_validator_under_sanitizers(codec_tool):
    out = subprocess.run([codec_tool], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DELTA-CODEC-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


@pytest.mark.parametrize("name", PAIR_NAMES)
def test_c_and_numpy_build_the_same_bytes(name, codec_tool, tmp_path):
    a, b, _ = all_pairs()[name]
    fa, fb, fd = (str(tmp_path / x) for x in ("before.bin", "after.bin", "delta.bin"))
    open(fa, "wb").write(S.build(a))
    open(fb, "wb").write(S.build(b))
    r = subprocess.run([codec_tool, "build", fa, fb, fd], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    delta = S.build_delta(a, b)
    assert open(fd, "rb").read() == delta, "the C++ and the numpy build_delta disagree"
    assert subprocess.run([codec_tool, "check", fd], capture_output=True, timeout=120).returncode == 0
    # ... and the C validator refuses what numpy refuses: a sealed blob with its first carried column broken.
    broken = bytearray(delta)
    broken[272 + 3] ^= 0x10
    fx = str(tmp_path / "broken.bin")
    open(fx, "wb").write(bytes(broken))
    assert subprocess.run([codec_tool, "check", fx], capture_output=True, timeout=120).returncode == 1
    with pytest.raises(S.FormatError):
        S.parse_delta(bytes(broken))
