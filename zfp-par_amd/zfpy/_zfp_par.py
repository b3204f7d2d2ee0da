"""Chunked parallel compression of a shared array: zfp_parallel.

Same surface as the reference's zfpy/_zfp_par.py (class zfp_p, :9-157):
a shared RawArray holds the field, zfp_chunkit partitions it into chunk boxes
(zfp_optimal_parts_from_size), compress() runs a ThreadPool over the chunks and
keeps one self-contained stream per chunk (whole-field header + the chunk's
blocks), decompress() writes every chunk back into the shared array.

On MI355X every chunk call runs on the GPU; the worker threads overlap the
host<->device copies and kernels of different chunks (each thread has its own
HIP stream).  Optional `ngpus=` spreads chunk i over device i % ngpus.
Divergences from the reference (bug fixes that do not change any output): the
decompress hand-off does not go through a module global (:144) and the JSON
helpers import json.  The block_size rule keeps the reference's 2^ndim.
"""
import json
import math
from multiprocessing import cpu_count
from multiprocessing.pool import ThreadPool
from multiprocessing.sharedctypes import RawArray

import numpy as np

from .zfpy_c import (_check_disjoint_blocks, _compress_portion, _compress_region_bytes, _compress_regions_bytes,
                     _decompress_portion, _decompress_region_stream,
                     _decompress_regions_stream, _fixed_rate, _region_box, device_count, zfp_chunkit)

_TYPECODE = {"float32": "f", "float64": "d", "int32": "i", "int64": "q"}
_ITEMSIZE = {"float32": 4, "float64": 8, "int32": 4, "int64": 8}


def _chunks_per_block(shape, dtype, est_compression_rate, block_size, nparts):
    """The reference constructor's partition argument (_zfp_par.py:40-60): blocks per chunk."""
    if dtype not in _TYPECODE:
        raise ValueError(f"Unsupported NumPy dtype: {dtype}")
    if len(shape) > 4:
        raise ValueError("Only support up to 4 dimensions")
    nblocks = 1
    for x in shape:
        nblocks *= int((x + 3) / 4)
    if block_size != -1:
        # 2^ndim (not 4^ndim) exactly as the reference (_zfp_par.py:55), so the partition matches
        compress_block_size = math.pow(2, len(shape)) * _ITEMSIZE[dtype] / est_compression_rate
        return block_size / compress_block_size
    if nparts != -1:
        return nblocks / nparts
    raise ValueError("Either block_size or nparts must be specified")


class zfp_p:
    def __init__(self, shape, dtype, est_compression_rate=3, method="BEST_CACHE", block_size=-1, nparts=-1,
                 ngpus=None):
        """Args as the reference: shape, numpy dtype name, estimated compression ratio, chunking method
        (BEST_CACHE or MAKE_EQUAL), approximate bytes per chunk (block_size) or number of parts (nparts).
        ngpus: spread chunks over this many HIP devices (default: 1, the current device)."""
        dtype = np.dtype(dtype).name
        chunks_per_block = _chunks_per_block(shape, dtype, est_compression_rate, block_size, nparts)
        n123 = 1
        for x in shape:
            n123 *= x
        self._raw_arr = RawArray(_TYPECODE[dtype], n123)
        self._np_array = np.frombuffer(self._raw_arr, dtype=dtype).reshape(shape)
        self._chunkit = zfp_chunkit(self._np_array, chunks_per_block, method)
        self._compress_data = []
        self._index_of = []  # (stream object, block-index blob) per chunk of the last compress()
        self._fixed = False  # the last compress() was fixed rate (compress_region)
        ndev = device_count()
        self._ngpus = max(1, min(ngpus or 1, ndev if ndev > 0 else 1))

    def get_raw_array(self):
        """Return raw array representation"""
        return self._raw_arr

    def get_numpy_array(self):
        """Return numpy array representation"""
        return self._np_array

    def get_chunkit(self):
        return self._chunkit

    def _device_of(self, ichunk):
        return ichunk % self._ngpus if self._ngpus > 1 else -1

    def compress(self, nthreads=-1, tolerance=-1, rate=-1, precision=-1):
        """Compress every chunk; result kept in self._compress_data (list of bytes, one per chunk).
        Chunk streams are plain bytes (as the reference's); a variable-rate chunk's GPU block index
        is kept beside its stream and used by decompress() while that stream object is the one
        compress() returned."""
        if nthreads == -1:
            nthreads = cpu_count()
        # The previous streams are dropped first: this object's references
        # would otherwise keep them alive (peak memory: two sets of streams)
        # until the new ones are assigned.  So a compress() that raises leaves
        # the object without compressed data (decompress() then raises too).
        self._compress_data, self._index_of = [], []
        self._fixed = _fixed_rate(tolerance, rate)
        tasks = [(i, tolerance, rate, precision) for i in range(self._chunkit.get_nchunks())]

        def one(i, tol, r, p):
            return _compress_portion(self._raw_arr, self._chunkit, i, tol, r, p, True, self._device_of(i), True)

        with ThreadPool(processes=max(1, min(nthreads, len(tasks) or 1))) as pool:
            res = pool.starmap(one, tasks)
        self._compress_data = [d for d, _ in res]
        self._index_of = [(d, blob) for d, blob in res]
        return self._compress_data

    def decompress(self, nthreads=-1):
        """Decompress every chunk stream into the shared array."""
        if nthreads == -1:
            nthreads = cpu_count()
        data = self._compress_data
        if len(data) != self._chunkit.get_nchunks():
            raise RuntimeError("no compressed data for this partition (call compress first)")

        def one(i):
            blob = getattr(data[i], "block_index", None)
            if blob is None and i < len(self._index_of) and self._index_of[i][0] is data[i]:
                blob = self._index_of[i][1]
            _decompress_portion(data[i], self._np_array, self._chunkit, i, self._device_of(i), blob)

        with ThreadPool(processes=max(1, min(nthreads, len(data) or 1))) as pool:
            pool.map(one, range(len(data)))

    def decompress_region(self, region, nthreads=-1):
        """The elements `region` of the compressed array as a new ndarray of the region's shape,
        decoding only the blocks that intersect it; the shared array is not touched.  region: one
        slice per axis in numpy order (step 1 or None, no negative indices; None: the whole axis).
        Every chunk whose box intersects the region decodes its part of it on the thread pool, with
        the chunk's kept block index, as decompress() does."""
        if nthreads == -1:
            nthreads = cpu_count()
        data = self._compress_data
        ck = self._chunkit
        if len(data) != ck.get_nchunks():
            raise RuntimeError("no compressed data for this partition (call compress first)")
        nd = ck.ndim
        box = _region_box(region, tuple(ck.ns_python))
        out = np.empty(tuple(e - f for f, e in box), dtype=ck.dtype)
        tasks = []
        for i in range(len(data)):
            coded = list(reversed(ck.boxes[i][:nd]))  # numpy axis order
            part = [(max(f, cf), min(e, ce)) for (f, e), (cf, ce) in zip(box, coded)]
            if all(f < e for f, e in part):
                tasks.append((i, coded, part))

        def one(i, coded, part):
            blob = getattr(data[i], "block_index", None)
            if blob is None and i < len(self._index_of) and self._index_of[i][0] is data[i]:
                blob = self._index_of[i][1]
            view = out[tuple(slice(f - f0, e - f0) for (f, e), (f0, _) in zip(part, box))]
            _decompress_region_stream(data[i], coded, part, view, self._device_of(i), blob)

        with ThreadPool(processes=max(1, min(nthreads, len(tasks) or 1))) as pool:
            pool.starmap(one, tasks)
        return out

    def decompress_regions(self, regions, nthreads=-1):
        """Many regions of the compressed array (each as for decompress_region) as a list of new
        ndarrays; the shared array is not touched.  Every chunk that any region touches makes one
        batched call on the thread pool for its parts of all the regions, each part written into its
        place in its region's array, with the chunk's kept block index."""
        if nthreads == -1:
            nthreads = cpu_count()
        data = self._compress_data
        ck = self._chunkit
        if len(data) != ck.get_nchunks():
            raise RuntimeError("no compressed data for this partition (call compress first)")
        nd = ck.ndim
        boxes = [_region_box(region, tuple(ck.ns_python)) for region in regions]
        outs = [np.empty(tuple(e - f for f, e in box), dtype=ck.dtype) for box in boxes]
        tasks = []
        for i in range(len(data)):
            coded = list(reversed(ck.boxes[i][:nd]))  # numpy axis order
            parts, views = [], []
            for box, out in zip(boxes, outs):
                part = [(max(f, cf), min(e, ce)) for (f, e), (cf, ce) in zip(box, coded)]
                if all(f < e for f, e in part):
                    parts.append(part)
                    views.append(out[tuple(slice(f - f0, e - f0) for (f, e), (f0, _) in zip(part, box))])
            if parts:
                tasks.append((i, coded, parts, views))

        def one(i, coded, parts, views):
            blob = getattr(data[i], "block_index", None)
            if blob is None and i < len(self._index_of) and self._index_of[i][0] is data[i]:
                blob = self._index_of[i][1]
            _decompress_regions_stream(data[i], coded, parts, views, self._device_of(i), blob)

        with ThreadPool(processes=max(1, min(nthreads, len(tasks) or 1))) as pool:
            pool.starmap(one, tasks)
        return outs

    def compress_region(self, region, values=None, nthreads=-1):
        """Code the elements `region` again, from `values` (an ndarray of the region's shape and the
        array's dtype; None: the shared array's own elements of the region), into the chunk streams the
        last fixed-rate compress() kept, without coding anything else: only the blocks that intersect
        the region are written.  Every chunk whose box intersects the region gets a new bytes object
        (the old stream with the region's blocks replaced), made on the thread pool, one chunk per
        task; the other chunks keep their stream objects.  Returns the list of chunk streams.
        Raises after a variable-rate compress() and when there is no compressed data."""
        if nthreads == -1:
            nthreads = cpu_count()
        data = self._compress_data
        ck = self._chunkit
        if len(data) != ck.get_nchunks():
            raise RuntimeError("no compressed data for this partition (call compress first)")
        if not self._fixed:
            raise RuntimeError("compress_region needs fixed-rate chunk streams (compress(rate=...)): in a "
                               "variable-rate stream a block of another length moves every later block")
        nd = ck.ndim
        box = _region_box(region, tuple(ck.ns_python))
        if values is None:
            values = self._np_array[tuple(slice(f, e) for f, e in box)]
        if not isinstance(values, np.ndarray):
            raise TypeError("values must be a numpy array")
        if values.dtype != np.dtype(ck.dtype):
            raise TypeError("values of dtype %s, the array holds %s" % (values.dtype, np.dtype(ck.dtype)))
        if values.shape != tuple(e - f for f, e in box):
            raise ValueError("values of shape %s, the region has shape %s"
                             % (values.shape, tuple(e - f for f, e in box)))
        tasks = []
        for i in range(len(data)):
            coded = list(reversed(ck.boxes[i][:nd]))  # numpy axis order
            part = [(max(f, cf), min(e, ce)) for (f, e), (cf, ce) in zip(box, coded)]
            if all(f < e for f, e in part):
                tasks.append((i, coded, part))

        def one(i, coded, part):
            view = values[tuple(slice(f - f0, e - f0) for (f, e), (f0, _) in zip(part, box))]
            return i, _compress_region_bytes(data[i], coded, part, view, self._device_of(i))

        with ThreadPool(processes=max(1, min(nthreads, len(tasks) or 1))) as pool:
            res = pool.starmap(one, tasks)
        for i, new in res:  # (all tasks succeeded: a failure leaves every stream as it was)
            data[i] = new
        return data

    def compress_regions(self, regions, values=None, nthreads=-1):
        """Code many regions again (each as for compress_region; values: a list of ndarrays, one per
        region, or None: the shared array's own elements), with one batched native call per touched
        chunk for that chunk's parts of all the regions, on the thread pool.  Every touched chunk gets
        one new bytes object, the other chunks keep their stream objects, and the streams are swapped
        only after every task succeeded.  Within one chunk no 4^d block (counted from the chunk's
        origin) may intersect the parts of two regions: ValueError, before any chunk is touched.
        Returns the list of chunk streams."""
        if nthreads == -1:
            nthreads = cpu_count()
        data = self._compress_data
        ck = self._chunkit
        if len(data) != ck.get_nchunks():
            raise RuntimeError("no compressed data for this partition (call compress first)")
        if not self._fixed:
            raise RuntimeError("compress_regions needs fixed-rate chunk streams (compress(rate=...)): in a "
                               "variable-rate stream a block of another length moves every later block")
        nd = ck.ndim
        boxes = [_region_box(r, tuple(ck.ns_python)) for r in regions]
        if values is None:
            values = [self._np_array[tuple(slice(f, e) for f, e in box)] for box in boxes]
        values = list(values)
        if len(values) != len(boxes):
            raise ValueError("%d value arrays for %d regions" % (len(values), len(boxes)))
        for k, (v, box) in enumerate(zip(values, boxes)):
            if not isinstance(v, np.ndarray):
                raise TypeError("values[%d] must be a numpy array" % k)
            if v.dtype != np.dtype(ck.dtype):
                raise TypeError("values[%d] of dtype %s, the array holds %s" % (k, v.dtype, np.dtype(ck.dtype)))
            if v.shape != tuple(e - f for f, e in box):
                raise ValueError("values[%d] of shape %s, its region has shape %s"
                                 % (k, v.shape, tuple(e - f for f, e in box)))
        tasks = []
        for i in range(len(data)):
            coded = list(reversed(ck.boxes[i][:nd]))  # numpy axis order
            parts, views, owner = [], [], []
            for k, box in enumerate(boxes):
                part = [(max(f, cf), min(e, ce)) for (f, e), (cf, ce) in zip(box, coded)]
                if all(f < e for f, e in part):
                    parts.append(part)
                    views.append(values[k][tuple(slice(f - f0, e - f0) for (f, e), (f0, _) in zip(part, box))])
                    owner.append(k)
            if parts:
                try:
                    _check_disjoint_blocks(parts, coded, "parts")
                except ValueError as err:
                    raise ValueError("chunk %d, regions %s: %s" % (i, owner, err)) from None
                tasks.append((i, coded, parts, views))

        def one(i, coded, parts, views):
            return i, _compress_regions_bytes(data[i], coded, parts, views, self._device_of(i))

        with ThreadPool(processes=max(1, min(nthreads, len(tasks) or 1))) as pool:
            res = pool.starmap(one, tasks)
        for i, new in res:  # (all tasks succeeded: a failure leaves every stream as it was)
            data[i] = new
        return data


def write_json_header(filename, dimensions, block_splits, compressed_files):
    """JSON sidecar: dimensions, per-axis split, compressed file name(s) (_zfp_par.py:159-175)."""
    header = {"dimensions": dimensions, "block_splits": block_splits, "compressed_files": compressed_files}
    with open(filename, "w") as f:
        json.dump(header, f, indent=4)


def read_json_header(filename):
    with open(filename, "r") as f:
        return json.load(f)
