"""The restated home slot of the digest index, the requestor index and the quota table
(tests/hash_index_cases.py) on the CPU: the inverse of the mix, the colliders, what a chain does when
the table doubles, the runs the GPU tests (tests/test_hash_index_gpu.py) rest on, and how far the keys
of the other suites ever get from their home slots. The stand-alone program
tests/native/hash_home_test.cc prints the library's own arithmetic (yadcc_amd/csrc/index_home.h) for
the same keys and sizes."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import hash_index_cases as H
from tests.conftest import ROOT

EDGE = [0, 1, 2, 3, H.M64, H.M64 - 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, 1 << 32, (1 << 32) - 1, 1 << 31, 1 << 30,
        1 << 27, 0xFFFFFFFF, 0x0A000000, 0x0B000000, H.C1, H.C2, 0x9E3779B97F4A7C15, 0xDEADBEEF00000001]


def sweep(n, seed):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(0, 1 << 64, n, dtype=np.uint64)]


def test_the_mix_and_its_inverse():
    """mix(unmix(y)) == y and unmix(mix(x)) == x on edge values, every single bit and a sweep; the
    published test vector of splitmix64 (seed 0: the first output is the finaliser of the increment)."""
    assert H.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert H.mix(0) == 0 and H.unmix(0) == 0
    vals = EDGE + [1 << b for b in range(64)] + [H.M64 ^ (1 << b) for b in range(64)] + sweep(20000, 1)
    for v in vals:
        assert H.mix(H.unmix(v)) == v and H.unmix(H.mix(v)) == v, hex(v)
    got = H.mix_np(np.array(vals, np.uint64))
    assert got.tolist() == [H.mix(v) for v in vals]


def test_the_slot_counts():
    for f in (H.slots_book, H.slots_requestor, H.slots_quota):
        assert [f(n) for n in (0, 1, 511, 512, 513, 1024, 1025, 2048, 2049, 4097)] == [
            1024, 1024, 1024, 1024, 2048, 2048, 4096, 4096, 8192, 16384]
    assert H.slots_book(1 << 30) == 1 << 31
    assert H.slots_requestor(1 << 33) == 1 << 31 and H.slots_quota((1 << 32) - 1) == 1 << 31
    assert H.bits_of(1024) == H.FLOOR_BITS


@pytest.mark.parametrize("bits", [10, 11, 13])
@pytest.mark.parametrize("h", H.HOMES + (0,))
def test_the_colliders_collide_and_are_distinct(bits, h):
    keys = H.key_colliders(bits, h, 600)
    assert len(set(keys)) == 600 and all(H.home(k, bits) == h for k in keys)
    assert H.ALL not in keys and 0 not in keys
    assert keys != sorted(keys), "the keys come scattered"
    both = {(H.mix(k) >> bits) & 1 for k in keys}
    assert both == {0, 1}
    n = 300 if bits == 10 else 40
    ips = H.ip_colliders(bits, h, n)
    assert len(set(ips)) == n and ips == sorted(ips) and all(0x0A000000 <= ip < 1 << 32 and H.home(ip, bits) == h for ip in ips)
    assert H.ip_colliders(bits, h, 5, skip=ips[:3]) == ips[3:8]


def test_zero_and_all_ones():
    """mix(0) == 0: key 0 lives at home 0 and comes only when asked for; all ones never comes."""
    assert H.home(0, 10) == 0
    keys = H.key_colliders(10, 0, 64, zero=True)
    assert keys[0] == 0 and len(set(keys)) == 64 and all(H.home(k, 10) == 0 for k in keys)
    with pytest.raises(AssertionError):
        H.key_colliders(10, 5, 4, zero=True)
    h1 = H.home(0xFFFFFFFF, 10)
    chain = [0xFFFFFFFF] + H.ip_colliders(10, h1, 63)
    assert len(set(chain)) == 64
    H.one_chain(chain, 10, h1)
    H.one_chain([0] + H.ip_colliders(10, 0, 63), 10, 0)
    # all ones as a digest key has a home like any other key; the book index never files it
    assert H.unmix(H.mix(H.ALL)) == H.ALL


@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("h", H.HOMES)
def test_stay_and_split_at_the_next_size(h, ids):
    """513 keys of one home at 1024 slots: where they are at 2048."""
    make = (lambda kind: H.ip_colliders(10, h, 513, kind=kind)) if ids else (lambda kind: H.key_colliders(10, h, 513, kind=kind))
    for kind, homes in (("stay0", {h: 513}), ("stay1", {h + 1024: 513}), ("split", {h: 257, h + 1024: 256})):
        keys = make(kind)
        assert len(set(keys)) == 513
        H.one_chain(keys[:512], 10, h)
        count = {}
        for k in keys:
            count[H.home(k, 11)] = count.get(H.home(k, 11), 0) + 1
        assert count == homes, (kind, count)
        occ, md = H.layout(keys, 11)
        want = frozenset().union(*[H.run_of(hh, n, 11) for hh, n in homes.items()])
        assert occ == want and md == max(homes.values()) - 1, kind
        if kind == "split":
            assert md == 256 and len(occ) == 513
        if kind == "stay1" and h >= 1021:
            assert 2047 in occ and 0 in occ, "the stayed chain crosses the wrap of the doubled table"


@pytest.mark.parametrize("n", H.LENGTHS + (512,))
@pytest.mark.parametrize("h", H.HOMES)
def test_a_chain_of_one_home_in_three_orders(h, n):
    """h .. h + n - 1 (mod slots), whatever the order; the wrap cases hold the last slot and slot 0."""
    keys = H.key_colliders(10, h, n)
    run = H.one_chain(keys, 10, h)
    rng = np.random.default_rng(n)
    for order in (sorted(keys), sorted(keys, reverse=True), [keys[i] for i in rng.permutation(n)]):
        assert H.layout(order, 10) == (run, n - 1)
    wraps = 1023 in run and 0 in run
    assert wraps == (h + n > 1024)
    if h == 1023 and n > 1:
        assert run == frozenset([1023]) | frozenset(range(n - 1)), "only the first member stays in the last slot"
    ips = H.ip_colliders(10, h, n)
    assert H.one_chain(ips, 10, h) == run
    # a key that is there already is found, not filed again
    assert H.layout(keys + keys[::-1], 10) == (run, n - 1)


@pytest.mark.parametrize("h", [100, 1010])
def test_two_touching_chains_form_one_run(h):
    """40 keys at h and 40 at h + 20: one run of 80, longer than either chain; a key is filed up to 79
    slots away (the first chain's last, behind the whole second chain) although its own chain has 40
    members."""
    a, b = H.key_colliders(10, h, 40), H.key_colliders(10, (h + 20) % 1024, 40)
    for order in (a + b, b + a, [k for pair in zip(a, b) for k in pair]):
        occ, md = H.layout(order, 10)
        assert occ == H.run_of(h, 80, 10)
        assert 39 < md <= 79
    assert H.layout(a + b, 10)[1] == 59 and H.layout(b + a, 10)[1] == 79
    assert (1023 in H.run_of(h, 80, 10) and 0 in H.run_of(h, 80, 10)) == (h == 1010)


def test_absent_keys_meet_the_run():
    for ids in (False, True):
        for h, n in ((100, 65), (1021, 257), (1023, 2), (1021, 1)):
            members = H.ip_colliders(10, h, n) if ids else H.key_colliders(10, h, n)
            out = H.absent_around(10, h, n, members, ids=ids)
            homes = [H.home(k, 10) for k in out]
            assert homes.count(h) >= 16 and (h + n) % 1024 in homes and len(set(out)) == len(out)
            if n > 2:
                assert (h + 1) % 1024 in homes and (h + n - 1) % 1024 in homes
            assert not set(out) & set(members)


# ---- how far the suites' keys get -----------------------------------------------------------------

def bound(n, slots):
    """A displacement of k means k consecutive slots that at least k keys call home. With n keys thrown at
    `slots` slots the number of keys of k given slots is binomial with mean a k, a = n / slots, and
    P(at least k) <= (a e^(1 - a))^k (Chernoff). Over all `slots` starts that is below 2^-20 from
    k = ln(slots 2^20) / -ln(a e^(1 - a)) on. The keys below are not random; they behave so if the mix is
    worth its name, and that is what the left column shows."""
    a = n / slots
    return math.ceil(math.log(slots * (1 << 20)) / -math.log(a * math.exp(1 - a)))


def suite_patterns():
    """(name, keys, slots): the key patterns of test_stream_book_find_gpu, _requestor_gpu, _quota_gpu and
    _fair_gpu, each in the smallest table its size allows."""
    for n in (64, 1025, 4097):
        yield "0x0B000000 + i, i < %d" % n, [0x0B000000 + i for i in range(n)], H.slots_quota(n)
    for m in (513, 2049):
        seq = [(i - 1) & H.M64 for i in range(1, m)]  # (all ones itself is never filed)
        yield "arange(%d) - 1" % m, seq, H.slots_book(m)
        yield "multiples of 2^32, %d" % m, [i << 32 for i in range(m)], H.slots_book(m)


def crafted():
    for n in (257, 512):
        yield "%d keys of home 1021" % n, H.key_colliders(10, 1021, n), 1024
    yield "512 ids of home 100", H.ip_colliders(10, 100, 512), 1024


def test_displacements_of_the_suites_keys_and_of_the_crafted_chains():
    """The two columns of the table in DESIGN 3.3.11."""
    for name, keys, slots in suite_patterns():
        hist = H.histogram(keys, H.bits_of(slots))
        most = max(d for d in hist if d != "wrap")
        b = bound(len(keys), slots)
        print("%-32s %6d slots: largest displacement %3d (bound %3d), at home %5.1f %%, crossed the wrap %d" % (
            name, slots, most, b, 100.0 * hist[0] / len(keys), hist.get("wrap", 0)))
        assert b < 128 and most <= b, (name, most, b)
        assert hist.get("wrap", 0) == 0, "the sequential keys never went from the last slot to slot 0"
    reached = {}
    for name, keys, slots in crafted():
        hist = H.histogram(keys, H.bits_of(slots))
        most = max(d for d in hist if d != "wrap")
        print("%-32s %6d slots: largest displacement %3d, crossed the wrap %d" % (name, slots, most, hist.get("wrap", 0)))
        assert all(hist[d] == 1 for d in range(len(keys)))
        reached[name] = (most, hist.get("wrap", 0))
    assert reached["257 keys of home 1021"] == (256, 254)
    assert reached["512 keys of home 1021"] == (511, 509)
    assert reached["512 ids of home 100"] == (511, 0)


# ---- against the library's own header -------------------------------------------------------------

def test_the_restatement_against_the_librarys_header_under_sanitizers(tmp_path):
    """tests/native/hash_home_test.cc includes only index_home.h; built the way the sanitizer programs of
    the Makefile are (`make hashhome`) and run as a program of its own: 10^4 keys, the crafted ones
    included, and every size in 0 .. 5000."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "hash_home_test")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "yadcc_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "hash_home_test.cc")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    keys = list(EDGE)
    for h in H.HOMES:
        keys += H.key_colliders(10, h, 257) + H.ip_colliders(10, h, 257) + H.key_colliders(11, h + 1024, 64, kind="stay1")
    keys += [0x0B000000 + i for i in range(1025)] + [i << 32 for i in range(513)]
    keys += sweep(10000 - len(keys), 2)
    assert len(keys) == 10000
    sizes = list(range(5001)) + [1 << 20, (1 << 20) + 1, 1 << 30]
    text = "".join("k %x\n" % k for k in keys) + "".join("s %d\n" % n for n in sizes)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    lines = out.stdout.split("\n")
    assert out.returncode == 0 and lines[len(keys) + len(sizes)] == "HASH-HOME-OK %d" % (len(keys) + len(sizes)), (
        out.stdout[-500:], out.stderr[-4000:])
    for k, line in zip(keys, lines):
        assert int(line, 16) == H.mix(k), "book_index_mix(%#x): the library %s, the restatement %#x" % (k, line, H.mix(k))
    for n, line in zip(sizes, lines[len(keys):]):
        assert [int(v) for v in line.split()] == [H.slots_book(n), H.slots_requestor(n), H.slots_quota(n)], (n, line)
