"""A call that fails after it queued work leaves its context fit for the next call.

libzfp_hip.so leases a device context (stream, scratch, 1 MiB of pinned
staging) to each call and hands the staging out afresh to the next call on
that context.  A variable-rate decompress into a host array with a non-unit x
stride queues the copy of its 4-byte index check word into the staging and
only then fails its host-side validation (copy_box: "needs unit x stride").
The lease synchronises the context's streams when a call ends that way, so
the next call on the same context stages into bytes nothing can still write.

This test pins the behaviour: the failed call fails as documented, and the
calls after it on the same thread (hence the same context) are bit-exact.  It
does not reproduce the race -- without the synchronise the stale 4-byte copy
has almost always landed before the next call stages; the soundness argument
is the lease's code (CtxLease in zfp-par_amd/csrc/hip).
"""
import numpy as np
import pytest

from pyoracle import params_precision

pytestmark = pytest.mark.gpu


def test_failed_decompress_leaves_context_usable(product, oracle):
    rng = np.random.default_rng(20)
    a = rng.standard_normal((8, 12, 16)).astype(np.float32)
    params = params_precision(16)  # variable rate: the check-word copy is staged
    words, end = oracle.compress_words(a, params)
    want = words.view(np.uint8).tobytes()[: (end + 63) // 64 * 8]
    ref, _ = oracle.decompress_words(words, a.shape, np.float32, params)

    got = product.compress(a, "precision", 16)
    index = product.last_index
    product.last_index = None
    try:
        assert got == want

        # a transposed host array: non-unit x stride, full field, no chunk
        out_t = np.zeros(a.shape[::-1], dtype=np.float32).T
        assert out_t.shape == a.shape and out_t.strides[-1] != out_t.itemsize
        _, n = product.decompress(got, a.shape, np.float32, "precision", 16, out=out_t, strided=True, index=index)
        assert n == 0
        assert b"unit x stride" in product.lib.zfp_hip_last_error()

        out, n = product.decompress(got, a.shape, np.float32, "precision", 16, index=index)
        assert n == len(got)
        assert out.tobytes() == ref.tobytes()

        assert product.compress(a, "precision", 16) == want
    finally:
        for idx in (index, product.last_index):
            if idx:
                product.lib.zfp_hip_index_free(idx)
        product.last_index = None
