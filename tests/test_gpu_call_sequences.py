"""Every ordered pair of catalogue calls, back to back on one device context.

A zfp_hip_* call borrows its context from a process-wide pool (most recently
returned first) and inherits what the previous call on it left: look-back
status words, partials, the overflow pool, staging that only grows, the scan's
index with its cached start table, the check word, pinned staging, the side
streams, the one-pair flags.  Correctness rests on each call resetting what it
reads; the rest of the suite orders calls by accident of collection order.

Here the catalogue of calls.py (about fifty small calls: every encoder and
decoder path, region and batched region calls, region encode, three calls
that fail, three through libzfp.so -- each with a CPU-made expected result) is
run along one Euler circuit of the complete directed graph over the entries,
so every ordered pair (i, j), (i, i) included, runs back to back exactly once;
three long random walks add histories deeper than two.  Each slice runs on
the test's thread after zfp_hip_release_scratch() and must hand back exactly
one context: had a second one served any call, the premise is gone and the
test fails.

ZFP_HIP_PIPE_MIN_MB=1 and ZFP_HIP_PIPE_SLAB_MB=1 hold for the whole module:
only the (64, 64, 80) float32 entries are that large, and every entry asserts
whether it took the slab pipeline.
"""
import os
import random

import pytest

import calls
from calls import euler_sequence, run_sequence, slices

pytestmark = pytest.mark.gpu

SEED = 20
NSLICES = 16
N = len(calls.build_catalogue())
SEQ = euler_sequence(N, SEED)
PARTS = slices(SEQ, NSLICES)
_PAIRS_RUN = set()


@pytest.fixture(scope="module")
def hip(product):
    return calls.load()


@pytest.fixture(scope="module")
def pipe_env():
    old = {k: os.environ.get(k) for k in calls.PIPE}
    os.environ.update(calls.PIPE)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def entries(hip, product, oracle, pipe_env):
    from capi import ZfpCAPI
    from pyoracle import REF_SO
    if not os.path.exists(REF_SO):  # (no entry may skip: the reference pin travels with the tree)
        pytest.fail("oracle/_ref is not built: the integer and libzfp entries have no expected results")
    out = calls.catalogue(oracle, ZfpCAPI(REF_SO))
    assert len(out) == N
    for e in out:
        e.setup(hip, product)
    yield out
    for e in out:
        e.teardown(hip)


def _run_on_one_context(hip, product, entries, seq):
    hip.zfp_hip_release_scratch()
    slot = calls.Slot(set_env=True)
    try:
        pairs = run_sequence(entries, seq, lambda e: e.run(hip, product, slot))
    finally:
        slot.close(hip)
    served = hip.zfp_hip_release_scratch()
    assert served == 1, "%d contexts served the calls of one thread: the sequence did not run on one context" % served
    return pairs


@pytest.mark.parametrize("k", range(NSLICES))
def test_every_ordered_pair(hip, product, entries, k):
    _PAIRS_RUN.update(_run_on_one_context(hip, product, entries, PARTS[k]))


def test_all_pairs_were_run(entries):
    """The union over the slices above (they run before this test) is every
    ordered pair of entries."""
    missing = {(i, j) for i in range(N) for j in range(N)} - _PAIRS_RUN
    print("pairs run: %d of %d" % (len(_PAIRS_RUN), N * N))
    assert not missing, ("%d of %d pairs were not run (a slice failed or was deselected)" % (len(missing), N * N),
                         [(entries[i].name, entries[j].name) for i, j in sorted(missing)[:5]])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_long_random_walks(hip, product, entries, seed):
    rng = random.Random(seed)
    _run_on_one_context(hip, product, entries, [rng.randrange(N) for _ in range(150)])
