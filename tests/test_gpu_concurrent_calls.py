"""Catalogue calls from eight host threads at once.

include/zfp_hip.h promises that distinct calls may run concurrently from
different host threads and that read-only streams, fields and indices may be
shared between them; zfpy's thread pool relies on both.  test_gpu_pool.py is
one call kind at one size.  Here the catalogue of calls.py runs from eight
threads (ctypes releases the GIL during a call, so the calls overlap):

  free mix            every thread walks its own permutation of the catalogue
                      twice with its own buffers; each entry's result and its
                      per-thread status (last scan, stale index, pipeline
                      signature, last error) must hold while the other threads
                      scan, fail and pipeline
  same call           all eight threads make one call from a barrier, five
                      rounds: the ticketed variable-rate encode, the overflow
                      redo, the scan, batched regions, region encode on private
                      streams, the slab pipeline; region decodes that share one
                      index with no start table yet (built once, read by all),
                      and full decodes that share one device stream and index
  neighbours          eight threads decode adjacent x-ranges of one field into
                      one host array, so neighbours write the same cache lines
                      and pages: region decodes at unaligned cuts, and
                      zfp_decompress_chunk through libzfp.so at block-aligned
                      cuts

The environment of a test is set before its threads start and restored after
the last has joined.  The three frozen sets are the pipeline knobs alone and
with the 3D and the 4D overflow-and-redo settings; an entry is left out of a
set only when the set's ZFP_HIP_SLOT_WORDS would apply to a kernel of the other
dimensionality (calls.allowed_in).  The pool must hand out between 2 and 8
contexts: 1 means nothing overlapped, more than 8 that the pool outgrew its
callers.  A thread that does not join in time counts as a hang.
"""
import ctypes
import os
import random
import threading
import time

import numpy as np
import pytest

import calls
from test_gpu_region import SENTINEL, _guarded, _job, _params, _region_decode
from test_gpu_stream_edges import _dense_job

pytestmark = pytest.mark.gpu

NTHREADS = 8
ROUNDS = 5
JOIN_SECONDS = 120
ENVS = {"pipe": dict(calls.PIPE), "pipe+redo3": dict(calls.PIPE, **calls.REDO3),
        "pipe+redo4": dict(calls.PIPE, **calls.REDO4)}


@pytest.fixture(scope="module")
def hip(product):
    return calls.load()


@pytest.fixture(scope="module")
def ref_lib():
    from capi import ZfpCAPI
    from pyoracle import REF_SO
    if not os.path.exists(REF_SO):  # (no entry may skip: the reference pin travels with the tree)
        pytest.fail("oracle/_ref is not built: the integer and libzfp entries have no expected results")
    return ZfpCAPI(REF_SO)


@pytest.fixture(scope="module")
def entries(hip, product, oracle, ref_lib):
    out = calls.catalogue(oracle, ref_lib)
    for e in out:
        e.setup(hip, product)
    yield out
    for e in out:
        e.teardown(hip)


def _set_env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    return old


def _restore_env(old):
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(params=list(ENVS))
def env(request):
    """One frozen environment: set before any thread starts, restored after all joined."""
    old = _set_env(ENVS[request.param])
    yield ENVS[request.param]
    _restore_env(old)


def _run_threads(body, what):
    """body(t, stop) on NTHREADS threads released from one barrier.  The first
    failure sets `stop` (checked between calls) and is raised here; a thread
    still alive after JOIN_SECONDS is a hang."""
    barrier = threading.Barrier(NTHREADS)
    stop = threading.Event()
    errors = []

    def run(t):
        try:
            barrier.wait(timeout=JOIN_SECONDS)
            body(t, stop)
        except BaseException as exc:  # noqa: BLE001 (reported by the main thread)
            errors.append((t, exc))
            stop.set()

    threads = [threading.Thread(target=run, args=(t,), daemon=True) for t in range(NTHREADS)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + JOIN_SECONDS
    for th in threads:
        th.join(timeout=max(0.0, deadline - time.monotonic()))
    alive = [i for i, th in enumerate(threads) if th.is_alive()]
    if alive:
        stop.set()
        pytest.fail("%s: threads %s did not finish within %d s (a hang)" % (what, alive, JOIN_SECONDS))
    if errors:
        real = [x for x in errors if not isinstance(x[1], threading.BrokenBarrierError)] or errors
        t, exc = real[0]
        raise AssertionError("%s: thread %d (%d threads failed): %s: %s" % (what, t, len(errors), type(exc).__name__,
                                                                          exc)) from exc


def _check_contexts(counts):
    """counts: {phase: contexts the pool handed back}.  Never more than the
    callers; and somewhere in the test calls overlapped."""
    print("contexts per phase:", counts)
    assert all(1 <= n <= NTHREADS for n in counts.values()), ("the pool outgrew its %d callers" % NTHREADS, counts)
    assert max(counts.values()) >= 2, ("no two calls overlapped: one context served everything", counts)


# ---------------------------------------------------------------------------
def test_free_mix(hip, product, entries, env):
    allowed = [e for e in entries if calls.allowed_in(e, env)]
    assert len(allowed) >= len(entries) - 12

    def body(t, stop):
        slot = calls.Slot(set_env=False)
        rng = random.Random(100 + t)
        try:
            for _ in range(2):
                order = list(allowed)
                rng.shuffle(order)
                for e in order:
                    if stop.is_set():
                        return
                    e.run(hip, product, slot)
        finally:
            slot.close(hip)

    hip.zfp_hip_release_scratch()
    _run_threads(body, "free mix")
    _check_contexts({"free mix": hip.zfp_hip_release_scratch()})


SAME_CALL = ["enc-f4-3d-prec18-host-index-off1-A", "enc-f8-3d-prec32-dev-exact-redo", "dec-f4-3d-prec18-scan-A",
             "regs-prec20-host-scan", "regs-rate12-dev-dev", "renc-rate3.25-off100-dev", "renc-rate8-host",
             "enc-pipe-prec18-index-off100", "dec-f4-3d-prec18-index-dev"]
SHARED_INDEX = "reg-prec20-caller-index"


def test_same_call_everywhere(hip, product, entries, env):
    by = {e.name: e for e in entries}
    counts = {}
    for name in SAME_CALL:
        e = by[name]
        if not calls.allowed_in(e, env):
            continue
        rounds = threading.Barrier(NTHREADS)

        def body(t, stop, e=e, rounds=rounds):
            slot = calls.Slot(set_env=False)
            try:
                for _ in range(ROUNDS):
                    rounds.wait(timeout=JOIN_SECONDS)
                    if stop.is_set():
                        rounds.abort()
                        return
                    e.run(hip, product, slot)
            except BaseException:
                rounds.abort()
                raise
            finally:
                slot.close(hip)

        hip.zfp_hip_release_scratch()
        _run_threads(body, name)
        counts[name] = hip.zfp_hip_release_scratch()

    # region decodes that share one index: a fresh one per round, with no start
    # table until the first calls of the round build it (once, under the lock)
    e = by[SHARED_INDEX]
    st = e.state
    job = _dense_job(calls.REGION_SHAPE, 3, st["params"])
    fresh = []
    try:
        for _ in range(ROUNDS):
            idx = hip.zfp_hip_index_create()
            fresh.append(idx)
            rc = hip.zfp_hip_index_build(ctypes.byref(job), st["words"].ctypes.data, len(st["words"]), 0, -1, idx)
            assert rc == 1, hip.zfp_hip_last_error().decode()
        rounds = threading.Barrier(NTHREADS)

        def body(t, stop):
            slot = calls.Slot(set_env=False)
            try:
                for r in range(ROUNDS):
                    rounds.wait(timeout=JOIN_SECONDS)
                    if stop.is_set():
                        rounds.abort()
                        return
                    slot.index_for[SHARED_INDEX] = fresh[r]
                    e.run(hip, product, slot)
            except BaseException:
                rounds.abort()
                raise
            finally:
                slot.close(hip)

        hip.zfp_hip_release_scratch()
        _run_threads(body, SHARED_INDEX + " (one fresh index per round)")
        counts[SHARED_INDEX] = hip.zfp_hip_release_scratch()
    finally:
        for idx in fresh:
            hip.zfp_hip_index_free(idx)
    _check_contexts(counts)


# ---------------------------------------------------------------------------
# neighbours in one host array
NEIGHBOUR_SHAPE = calls.REGION_SHAPE
REGION_CUTS = [0, 17, 33, 50, 66, 83, 99, 115, 130]
CHUNK_CUTS = [0, 16, 32, 48, 64, 80, 100, 116, 130]  # chunk decode needs block-aligned origins


@pytest.fixture
def pipe_env():
    old = _set_env(calls.PIPE)  # (float32 decoders read no slot knob: one set)
    yield
    _restore_env(old)


@pytest.mark.parametrize("mode,param", [("rate", 12), ("precision", 20)])
def test_neighbours_region_decode_into_one_host_array(hip, oracle, ref_lib, pipe_env, mode, param):
    a = calls.field(np.float32, NEIGHBOUR_SHAPE, "neighbours")
    ref = calls.reference(oracle, ref_lib, a, mode, param, 0)
    params = _params(mode, param, 3, 3)
    words = ref.words[:ref.exact].copy()
    job = _job(NEIGHBOUR_SHAPE, 3, params)
    big, view = _guarded(list(NEIGHBOUR_SHAPE), np.float32)
    strides = [s // 4 for s in view.strides]
    index = None
    if params[0] != params[1]:
        index = hip.zfp_hip_index_create()
        dense = _dense_job(NEIGHBOUR_SHAPE, 3, params)
        assert hip.zfp_hip_index_build(ctypes.byref(dense), words.ctypes.data, len(words), 0, -1, index) == 1
    nz, ny, _ = NEIGHBOUR_SHAPE

    def body(t, stop):
        x0, x1 = REGION_CUTS[t], REGION_CUTS[t + 1]
        dst = view[:, :, x0:x1]
        got = _region_decode(hip, job, [(0, nz), (0, ny), (x0, x1)], dst.ctypes.data, strides, words.ctypes.data,
                             len(words), 0, index)
        assert got == ((nz + 3) // 4) * ((ny + 3) // 4) * ((x1 - 1) // 4 - x0 // 4 + 1), (t, "blocks_read", got)
        assert hip.zfp_hip_last_scan(None, None) == 0 and hip.zfp_hip_last_stale_index() == 0, (t, "status")

    try:
        hip.zfp_hip_release_scratch()
        _run_threads(body, "region decodes of neighbouring x-ranges")
        served = hip.zfp_hip_release_scratch()
    finally:
        if index:
            hip.zfp_hip_index_free(index)
    assert 1 <= served <= NTHREADS, served
    assert np.ascontiguousarray(view).tobytes() == ref.decoded.tobytes(), "the shared array differs from the oracle's decode"
    view.view(np.uint8)[...] = SENTINEL
    assert (big.view(np.uint8) == SENTINEL).all(), "guard band written"


@pytest.mark.parametrize("mode,param", [("rate", 12), ("precision", 20)])
def test_neighbours_chunk_decode_into_one_host_array(hip, product, oracle, pipe_env, mode, param):
    from capi import ZfpCAPI
    a = calls.field(np.float32, NEIGHBOUR_SHAPE, "neighbours")
    params = _params(mode, param, 3, 3)
    nz, ny, _ = NEIGHBOUR_SHAPE
    want = np.zeros(NEIGHBOUR_SHAPE, dtype=np.float32)
    chunks = []
    for t in range(NTHREADS):
        box = [(CHUNK_CUTS[t], CHUNK_CUTS[t + 1]), (0, ny), (0, nz), (0, 0)]  # x first
        w, end = oracle.compress_words(a, params, box=box)
        dec, _ = oracle.decompress_words(w, NEIGHBOUR_SHAPE, np.float32, params, box=box)
        want[:, :, box[0][0]:box[0][1]] = dec[:, :, box[0][0]:box[0][1]]
        chunks.append((box[:3], w.tobytes()[:(end + 63) // 64 * 8]))
    big, view = _guarded(list(NEIGHBOUR_SHAPE), np.float32)
    apis = [ZfpCAPI(product.path) for _ in range(NTHREADS)]  # (ZfpCAPI keeps per-object state)

    def body(t, stop):
        box, data = chunks[t]
        _, n = apis[t].decompress(data, NEIGHBOUR_SHAPE, np.float32, mode, param, ztype=3, out=view, strided=True,
                                  chunk=box)
        assert n == len(data), (t, "bytes read", n, len(data), hip.zfp_hip_last_error().decode())

    hip.zfp_hip_release_scratch()
    _run_threads(body, "chunk decodes of neighbouring x-ranges")
    served = hip.zfp_hip_release_scratch()
    assert 1 <= served <= NTHREADS, served
    assert np.ascontiguousarray(view).tobytes() == want.tobytes(), "the shared array differs from the oracle's decode"
    view.view(np.uint8)[...] = SENTINEL
    assert (big.view(np.uint8) == SENTINEL).all(), "guard band written"
