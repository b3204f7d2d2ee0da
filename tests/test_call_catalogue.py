"""The call catalogue (calls.py) checked without a GPU, before it is trusted on one.

  * euler_sequence / slices: every ordered pair exactly once, nothing lost at
    the cuts, deterministic per seed
  * every entry's prepare runs; the oracle's expected stream of every float
    entry equals the reference library's for the same call
  * run_sequence is sensitive: a stub library that answers every call from the
    entry's own expected result passes, and the same stub with one fault --
    the previous call's output returned for one entry, one bit flipped past
    the stream's end, zfp_hip_last_scan left from the previous call -- fails at
    the position where the fault first shows, with the pair named.  This
    stands in for a mutation run on the GPU.
"""
import ctypes

import numpy as np
import pytest

import calls
import streams
from calls import SequenceFailure, euler_sequence, pairs_of, run_sequence, slices
from test_gpu_region import TYPES


@pytest.fixture(scope="module")
def entries(oracle, ref_capi):
    return calls.catalogue(oracle, ref_capi)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, len(calls.build_catalogue())])
def test_euler_sequence_has_every_ordered_pair_once(n):
    seq = euler_sequence(n, 3)
    assert len(seq) == n * n + 1 and seq[0] == seq[-1]
    pairs = pairs_of(seq)
    assert len(set(pairs)) == len(pairs) == n * n
    assert set(pairs) == {(i, j) for i in range(n) for j in range(n)}
    assert seq == euler_sequence(n, 3), "not deterministic per seed"
    if n > 2:
        assert seq != euler_sequence(n, 4), "the seed does not matter"
    for k in (1, 2, 5, 12):
        parts = slices(seq, k)
        assert len(parts) == max(1, min(k, n * n))
        assert all(a[-1] == b[0] for a, b in zip(parts, parts[1:]))
        joined = [p for part in parts for p in pairs_of(part)]
        assert joined == pairs, (n, k, "the slices lose or repeat a pair")


def test_entries_prepare_and_names_are_unique(entries):
    assert len(entries) >= 35
    assert len({e.name for e in entries}) == len(entries)
    assert all(e.state is not None for e in entries)
    kinds = {e.kind for e in entries}
    assert kinds == {"encode", "decode", "decode-stale", "region", "regions", "region-encode", "fails", "capi"}
    assert sum(e.scans for e in entries) >= 8 and sum(e.stale for e in entries) == 1
    assert sum(e.pipelined for e in entries) == 4 and sum(bool(e.fails) for e in entries) == 3


def test_float_streams_of_the_oracle_equal_the_reference_library(entries, ref_capi):
    checked = 0
    for e in entries:
        st = e.state
        if e.kind not in ("encode", "decode") or st["a"].dtype.kind != "f":
            continue
        a, ref = st["a"], st["ref"]
        data = ref_capi.compress(np.array(a), st["mode"], st["param"], ztype=TYPES[a.dtype], pad_bits=st["off"])
        assert data == ref.words[:ref.exact].tobytes(), e.name
        dec, _ = ref_capi.decompress(data, a.shape, a.dtype, st["mode"], st["param"], ztype=TYPES[a.dtype],
                                     pad_bits=st["off"])
        assert dec.tobytes() == ref.decoded.tobytes(), e.name
        checked += 1
    assert checked >= 25


def test_frozen_environment_sets_leave_out_the_other_dimensionality(entries):
    by = {e.name: e for e in entries}
    redo3 = dict(calls.PIPE, **calls.REDO3)
    redo4 = dict(calls.PIPE, **calls.REDO4)
    assert all(calls.allowed_in(e, calls.PIPE) for e in entries)
    assert not calls.allowed_in(by["enc-f4-4d-rev-index-redo"], redo3)
    assert calls.allowed_in(by["enc-f8-3d-prec32-dev-exact-redo"], redo3)
    assert not calls.allowed_in(by["enc-f8-3d-prec32-dev-exact-redo"], redo4)
    assert not calls.allowed_in(by["dec-f8-3d-prec32-scan-dev"], redo4)   # short_stage_words: 3D f64, maxprec <= 32
    assert not calls.allowed_in(by["enc-pipe-prec18-index-off100"], redo4)
    assert calls.allowed_in(by["enc-f4-4d-rev-index-redo"], redo4)
    for name in ("enc-f4-3d-rate16-dev-dev-large", "enc-f4-4d-rate3.25", "enc-i4-2d-prec12", "dec-f4-4d-rev-scan",
                 "reg-prec20-scan-A", "renc-rate8-dev"):
        assert calls.allowed_in(by[name], redo3) and calls.allowed_in(by[name], redo4), name


# ---------------------------------------------------------------------------
# the runner against a stub library
def _words_at(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_uint64 * n).from_address(ptr))


def _resized(data, n):
    data = bytes(data) or b"\0"
    return (data * (n // len(data) + 1))[:n]


class Stub:
    """zfp_hip_compress / zfp_hip_decompress answered from the current entry's
    expected result (`entry` is set by the caller), with the per-thread status
    a right library reports, and optionally one fault on calls of `target`."""

    def __init__(self, fault=None, target=None):
        self.fault, self.target = fault, target
        self.entry = None
        self.scan, self.timed, self.pipe = 0, False, False
        self.last = b""
        self.handles = 0

    def _faulty(self, fault):
        return self.fault == fault and self.entry.name == self.target

    def _status(self, scan):
        if not self._faulty("stale-scan"):
            self.scan = 1 if scan else 0
        self.timed, self.pipe = True, self.entry.pipelined

    def zfp_hip_index_create(self):
        self.handles += 1
        return self.handles

    def zfp_hip_index_free(self, idx):
        pass

    def zfp_hip_index_build(self, jobref, wptr, cap, off, dev, idx):
        return 1

    def zfp_hip_last_scan(self, ms, passes):
        return self.scan

    def zfp_hip_last_stale_index(self):
        return 0

    def zfp_hip_last_error(self):
        return b""

    def zfp_hip_last_timing(self, kref, tref):
        if not self.timed:
            return 0
        kref._obj.value = 0.0 if self.pipe else 0.25
        tref._obj.value = 1.0
        return 1

    def zfp_hip_compress(self, jobref, fptr, wptr, cap, off, head, dev, index, endref):
        ref = self.entry.state["ref"]
        self._status(False)
        mem = _words_at(wptr, cap + 1)  # (one word past the capacity: the trailing guard)
        img = streams.expected_image(mem[:cap], off, head, ref.words, ref.end_bit)
        payload = img[off // 64:ref.exact].tobytes()
        if self._faulty("previous"):
            payload = _resized(self.last, len(payload))
        mem[off // 64:ref.exact] = np.frombuffer(payload, dtype=np.uint64)
        if self._faulty("bitflip"):
            mem[ref.exact] ^= np.uint64(1 << 17)
        self.last = payload
        endref._obj.value = ref.end_bit
        return 1

    def zfp_hip_decompress(self, jobref, dptr, wptr, cap, off, dev, index, endref):
        st = self.entry.state
        self._status(not st["fixed"] and not index)
        payload = st["ref"].decoded.tobytes()
        if self._faulty("previous"):
            payload = _resized(self.last, len(payload))
        ctypes.memmove(dptr, payload, len(payload))
        self.last = payload
        endref._obj.value = st["ref"].end_bit
        return 1


@pytest.fixture
def stubbed(entries, monkeypatch):
    """The entries the stub answers (plain encodes and decodes), set up on host
    memory standing in for the device; run(stub, seq) drives run_sequence."""
    monkeypatch.setattr(calls, "FAKE_DEVICE", True)
    sub = [e for e in entries if e.kind in ("encode", "decode")]
    setup_stub = Stub()
    for e in sub:
        e.setup(setup_stub, None)

    def run(stub, seq):
        slot = calls.Slot(set_env=False)

        def call(e):
            stub.entry = e
            e.run(stub, None, slot)
        try:
            return run_sequence(sub, seq, call)
        finally:
            slot.close(stub)

    yield sub, run
    for e in sub:
        e.teardown(setup_stub)


def _first(seq, sub, target, shows):
    """The first position of `target` whose predecessor makes the fault show."""
    t = [e.name for e in sub].index(target)
    return next(p for p in range(len(seq)) if seq[p] == t and shows(sub[seq[p - 1]] if p else None))


def test_stub_library_passes_every_pair(stubbed):
    sub, run = stubbed
    seq = euler_sequence(len(sub), 11)
    assert run(Stub(), seq) == {(i, j) for i in range(len(sub)) for j in range(len(sub))}


@pytest.mark.parametrize("fault,target,shows,says", [
    ("previous", "dec-f4-3d-rate16-host", lambda prev: prev is None or prev.name != "dec-f4-3d-rate16-host", "destination differs"),
    ("previous", "enc-f4-3d-rate8-host-host-off64", lambda prev: prev is None or prev.name != "enc-f4-3d-rate8-host-host-off64",
     "stream bits"),
    ("bitflip", "enc-f4-3d-rate3.25-dev-dev-off100", lambda prev: True, "after the stream, inside the capacity"),
    ("bitflip", "enc-pipe-rate3.25-off100", lambda prev: True, "past the capacity"),
    ("stale-scan", "dec-f4-3d-rate16-dev", lambda prev: prev is not None and prev.scans, "zfp_hip_last_scan"),
    ("stale-scan", "dec-f4-3d-prec18-scan-A", lambda prev: prev is None or not prev.scans, "zfp_hip_last_scan"),
])
def test_runner_reports_a_faulty_stub_at_the_right_position(stubbed, fault, target, shows, says):
    sub, run = stubbed
    seq = euler_sequence(len(sub), 11)
    pos = _first(seq, sub, target, shows)
    with pytest.raises(SequenceFailure) as info:
        run(Stub(fault, target), seq)
    msg = str(info.value)
    prev = sub[seq[pos - 1]].name if pos else "(nothing)"
    assert msg.startswith("position %d of %d: %s failed" % (pos, len(seq), target)), msg
    assert "(pair %s -> %s)" % (prev, target) in msg, msg
    assert says in msg, msg
    before = [sub[j].name for j in seq[max(0, pos - 3):pos]]
    assert repr(before) in msg, msg


def test_refusal_before_any_gpu_call_runs_without_a_gpu(entries):
    """The 4D region refusal is decided before any GPU call: the entry, its
    untouched destination and stream and its per-thread status (no scan, no
    timing, the error names the call) hold against the real library here."""
    hip = calls.load()
    e = next(e for e in entries if e.name == "fail-region-4d")
    slot = calls.Slot(set_env=False)
    for _ in range(2):
        e.run(hip, None, slot)
