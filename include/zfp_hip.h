/*
 * zfp_hip.h -- C-ABI of the MI355X (gfx950) codec library libzfp_hip.so.
 *
 * This is the seam the host C library (libzfp.so, include/zfp.h) calls for the
 * data-parallel hot path.  Plain pointers and sizes only: no HIP, torch or C++
 * types cross it, so any FFI (ctypes, cffi, Cython, cgo, JNI) can bind it.
 *
 * What each entry point replaces in the reference (SEP-software/zfp-par):
 *
 *   zfp_hip_compress    the execution-policy table slot of zfp_compress_call
 *                       (src/zfp.c:1510-1564) -> compress_strided_<T>_3/_4
 *                       (src/template/compress.c:67-153), i.e. the raster block
 *                       traversal plus the per-block codec of
 *                       src/template/{encodef,encode,encode3,encode4,revencode*}.c
 *   zfp_hip_decompress  the slot of zfp_decompress_call (src/zfp.c:1605-1649) ->
 *                       decompress_strided_<T>_3/_4 (src/template/decompress.c:66-140)
 *                       with the decoders of src/template/{decodef,decode,...}.c
 *   zfp_hip_index_*     no reference equivalent: variable-rate streams carry no
 *                       block offsets (docs execution.rst).  The GPU encoder can
 *                       emit a side-band block index; without one (a stream
 *                       from the reference, a file, another process) the
 *                       decoder first finds the block starts with a parallel
 *                       resynchronising parse of the stream (zfp_hip_index_build),
 *                       which replaces the serial block walk of
 *                       src/template/decompress.c:66-140.
 *
 * Memory: `field_base` and `words` may each be host or device (hipMalloc)
 * memory; the library stages host buffers through device memory itself.
 * Threading: distinct calls may run concurrently from different host threads.
 * Each call (not each thread) borrows a context -- a HIP stream and scratch --
 * from a process-wide pool and returns it when it ends, so consecutive calls of
 * one thread usually reuse one context and concurrent calls never share one.
 * Concurrent calls may share what they only read: a stream being decoded, a
 * field being encoded, and an index (the start table a region decode makes
 * from it is built once, under a lock).  What a call writes -- the destination
 * field, the stream or index an encode fills -- belongs to that call alone;
 * in particular two region encodes on one stream at the same time are not
 * supported.  The last-error, last-timing, last-scan and stale-index queries
 * answer for the calling thread's most recent call, a refused one included.
 * Errors: entry points return 0 on failure (unsupported type/dimensionality,
 * capacity too small, HIP error); zfp_hip_last_error() describes the failure.
 */
#ifndef ZFP_HIP_H
#define ZFP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One (de)compression job: field geometry, chunk box, codec parameters. */
typedef struct zfp_hip_job {
  int32_t type;        /* zfp_type: 1 = int32, 2 = int64, 3 = float, 4 = double */
  int32_t dims;        /* 1 .. 4 */
  uint64_t n[4];       /* field extents, x first (zfp_field nx..nw) */
  int64_t s[4];        /* element strides, resolved (zfp_field_stride) */
  uint64_t f[4];       /* chunk box first element per axis (zfp_chunk fx..fw) */
  uint64_t e[4];       /* chunk box exclusive end per axis (zfp_chunk ex..ew) */
  uint32_t minbits;    /* zfp_stream parameters (zfp.h:90-97) */
  uint32_t maxbits;
  uint32_t maxprec;
  int32_t minexp;
} zfp_hip_job;

typedef struct zfp_hip_index zfp_hip_index;

/* Number of visible HIP devices (0 when no GPU or no driver). */
int zfp_hip_device_count(void);

/* Human-readable description of the last failure on this thread. */
const char* zfp_hip_last_error(void);

/* 1 if p points into HIP device memory (0 without a GPU).  The host bitstream
 * (stream_open) uses it to move the words it touches itself with hipMemcpy. */
int zfp_hip_is_device_ptr(const void* p);
/* Synchronous copy between any host/device pointers; 0 on failure. */
int zfp_hip_memcpy(void* dst, const void* src, size_t bytes);

/*
 * Encode the chunk box of `job` into the stream whose word array begins at
 * `words` (capacity `capacity_words` 64-bit words), starting at bit
 * `bit_offset`.  `head_word` holds the stream bits already written below
 * bit_offset in word bit_offset/64 (the bitstream's pending buffer).
 * On success the stream is written through the last partial word, which is
 * zero-padded (flushed); *end_bit receives the bit position after the last
 * block.  For variable-rate modes, `index` (optional) receives the block index.
 */
int zfp_hip_compress(const zfp_hip_job* job, const void* field_base, uint64_t* words,
                     uint64_t capacity_words, uint64_t bit_offset, uint64_t head_word,
                     int device, zfp_hip_index* index, uint64_t* end_bit);

/*
 * Decode the chunk box of `job` from the stream at `words` (readable capacity
 * `capacity_words`), starting at bit `bit_offset`; *end_bit receives the bit
 * position after the last block.  For variable-rate modes `index` is used when
 * it was made for this block count, layout and bit offset (zfp_hip_compress or
 * zfp_hip_index_build); otherwise (or when NULL) the stream is scanned first.
 */
int zfp_hip_decompress(const zfp_hip_job* job, void* field_base, const uint64_t* words,
                       uint64_t capacity_words, uint64_t bit_offset, int device,
                       const zfp_hip_index* index, uint64_t* end_bit);

/*
 * Region decode: write the elements [lo, hi) of the field -- any sub-box of the
 * coded box [f, e) of `job`, element-granular, f <= lo < hi <= e per axis --
 * exactly as zfp_hip_decompress of the whole box would, decoding only the
 * blocks that intersect the region.  `job` gives the coded box and the codec
 * parameters (job->s is not used); the stream's first block is at bit
 * `bit_offset` of `words`.  `dst` (host or device memory) receives element x
 * at dst[sum over axes of (x - lo) * dst_stride] (element strides; entries of
 * lo, hi and dst_stride from job->dims on are not read); nothing else is
 * written.  1D to 3D; a 4D job returns 0.  A null pointer, an empty region or
 * one outside the coded box, a 4D job and more than 2^32 - 1 region blocks
 * return 0 before any GPU call, with `dst` untouched.
 * Variable rate: `index` as for zfp_hip_decompress (NULL or not made for this
 * stream: the stream is scanned first); the decoded length of every block read
 * is checked against the index, and a stale index is replaced by a scan
 * (zfp_hip_last_stale_index).  The per-block start table made from the index
 * is kept in it for later calls.
 * Host `words`: a fixed-rate call copies to the device only the words from the
 * first needed block's start to the last needed block's end (plus one word of
 * look-ahead); a variable-rate call stages the whole stream, as
 * zfp_hip_decompress does.
 * *blocks_read (optional) receives the number of blocks staged and decoded:
 * the product over axes of (hi - 1 - f) / 4 - (lo - f) / 4 + 1.
 * zfp_hip_last_timing reports the region kernel as it does any decode.
 */
int zfp_hip_decompress_region(const zfp_hip_job* job, const uint64_t lo[4], const uint64_t hi[4],
                              void* dst, const int64_t dst_stride[4],
                              const uint64_t* words, uint64_t capacity_words, uint64_t bit_offset,
                              int device, const zfp_hip_index* index, uint64_t* blocks_read);

/* One region of a batch (zfp_hip_decompress_regions). */
typedef struct zfp_hip_region {
  uint64_t lo[4], hi[4];   /* as zfp_hip_decompress_region */
  void* dst;               /* host or device memory */
  int64_t dst_stride[4];   /* element strides */
} zfp_hip_region;

/*
 * Batched region decode: `nregions` sub-boxes of the coded box of `job`, each
 * into its own destination, in one kernel launch (the regions' blocks are
 * dealt out to the launch's waves, whole waves per region).  Region i receives
 * exactly what zfp_hip_decompress_region writes for (lo, hi, dst, dst_stride)
 * of regions[i] -- bit for bit what a full decode holds there -- and nothing
 * else is written.  Regions may overlap each other and may repeat (a block two
 * regions touch is decoded twice); destinations that overlap each other are the
 * caller's error and are not checked.  The destinations of one call are all
 * host or all device memory: a mix returns 0 before any launch or copy.
 * Checked before any GPU call, returning 0 with no destination written and
 * *blocks_read untouched: a null `job`, `regions` or `words`, a null `dst` in
 * any entry, any entry's region empty or outside the coded box (the message
 * names the entry), a 4D job, more than 65,536 regions, and more than
 * 2^32 - 1 lanes once every region is padded to whole waves of 64 blocks.  One
 * bad entry fails the whole call.  nregions == 0 returns 1 with
 * *blocks_read = 0 and makes no GPU call.
 * Variable rate: `index` as for zfp_hip_decompress_region; a stale index
 * repeats the whole batch with a scan (zfp_hip_last_stale_index).
 * Host `words`: a fixed-rate call stages one span, from the first word of the
 * lowest block any region needs to the last word of the highest plus one word
 * of look-ahead -- for regions that lie far apart that is most of the stream;
 * streams in device memory are the fast path.  A variable-rate host stream is
 * staged whole.  Host destinations: the regions are decoded into dense device
 * images and copied out one by one.
 * *blocks_read (optional) receives the sum over the regions of
 * zfp_hip_decompress_region's block count (padding lanes are not counted).
 * zfp_hip_last_timing reports the one launch.
 */
int zfp_hip_decompress_regions(const zfp_hip_job* job, const zfp_hip_region* regions, uint64_t nregions,
                               const uint64_t* words, uint64_t capacity_words, uint64_t bit_offset,
                               int device, const zfp_hip_index* index, uint64_t* blocks_read);

/*
 * Region encode: rewrite the sub-box [lo, hi) (element granular, f <= lo < hi
 * <= e per axis) of the fixed-rate stream that codes the chunk box of `job`,
 * in place.  `src` (host or device memory) holds element x of the region at
 * src[sum over axes of (x - lo) * src_stride] (element strides; job->s is not
 * used).  After the call every block that intersects the region holds exactly
 * the bits zfp_hip_compress would write for it from the image: the field as a
 * full decode of the old stream gives it, with the region's elements replaced
 * by the source.  A block whose elements inside the field all lie in the
 * region is coded from the source alone and its old bits are never read; a
 * block the region cuts through (or one at a chunk end that is neither a
 * multiple of 4 from the chunk's origin nor the field's edge) is decoded,
 * overlaid and coded again, so the elements it keeps go through one more lossy
 * round.  Every other bit of the stream is left as it was: blocks that do not
 * intersect the region, bits below `bit_offset`, bits past the last block,
 * words past the stream.
 * 1D to 3D, fixed rate only (in a variable-rate stream a block of another
 * length would move every later block).  A null pointer, an empty region or
 * one outside the coded box, a 4D job, a variable-rate job, more than
 * 2^32 - 1 region blocks and a stream whose `capacity_words` ends before the
 * last needed block's last bit return 0 before any GPU call, with the stream
 * untouched.
 * Host `words`: the words from the first needed block's first word to the
 * last needed block's last word are copied to the device, merged there and
 * copied back; for a thin region across a large stream (an x slice) that span
 * is nearly the whole stream -- streams in device memory are the fast path.
 * Two calls on one stream at the same time are not supported.
 * *blocks_written (optional) receives the number of blocks coded: the product
 * formula of zfp_hip_decompress_region's blocks_read.
 * zfp_hip_last_timing reports the region kernel as it does any encode.
 */
int zfp_hip_compress_region(const zfp_hip_job* job, const uint64_t lo[4], const uint64_t hi[4],
                            const void* src, const int64_t src_stride[4],
                            uint64_t* words, uint64_t capacity_words, uint64_t bit_offset,
                            int device, uint64_t* blocks_written);

/* One region of a batch (zfp_hip_compress_regions). */
typedef struct zfp_hip_src_region {
  uint64_t lo[4], hi[4];    /* as zfp_hip_compress_region */
  const void* src;          /* host or device memory */
  int64_t src_stride[4];    /* element strides */
} zfp_hip_src_region;

/*
 * Batched region encode: `nregions` sub-boxes of the coded box of `job`, each
 * from its own source, rewritten in place in one kernel launch (the regions'
 * blocks are dealt out to the launch's waves, whole waves per region).  After
 * the call the stream holds what one zfp_hip_compress_region call per entry,
 * in any order, would leave: every block that intersects a region holds the
 * bits zfp_hip_compress writes for it from the image (a full decode of the
 * old stream with that region's elements replaced); covered blocks are coded
 * from the source alone, partly covered ones are decoded, overlaid and coded
 * again; every other bit is untouched -- other blocks, bits below
 * `bit_offset`, bits past the last block, words past the stream.
 * The block sets of the entries must be pairwise disjoint: two entries that
 * intersect a common 4^d block (blocks count from the coded box's origin) are
 * refused, with a message that names both, even if their elements are
 * disjoint.  The merge into the stream relies on no block's bits being read
 * by any wave but its own, before that wave's writes; that holds across
 * regions exactly when no block belongs to two of them.  A shared block would
 * be read by one wave while another rewrites it, and the result would depend
 * on the entries' order.  Blocks of different entries that share a stream
 * word (rate 3.25, a 96-bit header) are fine.  A caller with adjacent tiles
 * that do not lie on multiples of 4 from the coded box's origin merges them
 * or makes two calls.
 * These return 0 before any GPU call, with the stream and *blocks_written
 * untouched: a null `job`, `regions` or `words`, a null `src` in any entry,
 * any entry's region empty or outside the coded box (the message names the
 * entry), a 4D job, a variable-rate job, more than 65,536 regions, more than
 * 2^32 - 1 lanes once every region is padded to whole waves of 64 blocks, a
 * stream whose `capacity_words` ends before the last bit of the highest block
 * any entry needs, and two entries that share a block.  One bad entry fails
 * the whole call.  nregions == 0 returns 1 with *blocks_written = 0 and makes
 * no GPU call.  The sources are all in host or all in device memory; a
 * mixture returns 0 before any launch or copy.
 * Host `words`: one span is staged, from the first word of the lowest block
 * any region needs to the last word of the highest, merged on the device and
 * copied back whole -- for regions that lie far apart that is most of the
 * stream; streams in device memory are the fast path.  Host sources are
 * packed into dense device images.  Two calls on one stream at the same time
 * are not supported.
 * *blocks_written (optional) receives the sum over the entries of
 * zfp_hip_compress_region's block count (padding lanes are not counted).
 * zfp_hip_last_timing reports the one launch.
 */
int zfp_hip_compress_regions(const zfp_hip_job* job, const zfp_hip_src_region* regions, uint64_t nregions,
                             uint64_t* words, uint64_t capacity_words, uint64_t bit_offset,
                             int device, uint64_t* blocks_written);

/*
 * Build the block index of the variable-rate stream at `words` for the chunk
 * box of `job`, blocks starting at bit `bit_offset` (a parallel parse of the
 * stream on the GPU; see scan.h).  Returns 0 for fixed-rate jobs, truncated
 * streams or HIP errors.
 */
int zfp_hip_index_build(const zfp_hip_job* job, const uint64_t* words, uint64_t capacity_words,
                        uint64_t bit_offset, int device, zfp_hip_index* index);

/* Block index (variable-rate streams). */
zfp_hip_index* zfp_hip_index_create(void);
void zfp_hip_index_free(zfp_hip_index* index);
uint64_t zfp_hip_index_blocks(const zfp_hip_index* index);
/* serialise to / restore from host bytes (returns bytes written / NULL) */
size_t zfp_hip_index_export(const zfp_hip_index* index, void* buffer, size_t capacity);
zfp_hip_index* zfp_hip_index_import(const void* buffer, size_t bytes);
/* start bit of every block relative to block 0, in stream (raster block)
 * order, then the bit after the last: offsets[0 .. nblocks] (count >=
 * nblocks + 1; offsets NULL: returns nblocks + 1).  Returns the entries
 * written, 0 on failure.  The random access into a variable-rate stream that
 * the reference keeps in its compressed arrays' block index (zfp/index.hpp). */
uint64_t zfp_hip_index_offsets(const zfp_hip_index* index, uint64_t* offsets, uint64_t count);
/* Fill `index` (from zfp_hip_index_create; its device buffers are reused) for
 * the chunk box of `job` -- `count` blocks whose stream offsets the caller
 * knows (offsets[0 .. count], bits, any common origin), the first at bit
 * `bit_offset` of `words` -- so zfp_hip_decompress decodes them without
 * scanning the stream.  The random access of the reference's compressed
 * arrays (a cache line's blocks, constarray3.hpp via index.hpp).  1 on success. */
int zfp_hip_index_set_offsets(zfp_hip_index* index, const zfp_hip_job* job, const uint64_t* words,
                              uint64_t capacity_words, uint64_t bit_offset, const uint64_t* offsets, uint64_t count,
                              int device);

/*
 * Timing of the most recent zfp_hip_compress/zfp_hip_decompress on this
 * thread, from HIP events recorded on the stream the kernels ran on:
 * kernel_ms = the codec kernel alone, total_ms = everything enqueued by the
 * call (staging copies, fix-ups, kernel).  A compress whose field and stream
 * are both in device memory and that queues the codec kernel alone (aligned
 * fixed rate at a word-aligned start) records one event pair: total_ms is then
 * equal to kernel_ms.  Returns 0 if no call has run.
 */
int zfp_hip_last_timing(double* kernel_ms, double* total_ms);

/* Index scan of the most recent call on this thread (decompress without a
 * matching index, or zfp_hip_index_build): its duration from HIP events and
 * the number of segment passes.  Returns 0 if that call did not scan. */
int zfp_hip_last_scan(double* scan_ms, int* passes);

/* 1 if the most recent zfp_hip_decompress on this thread was handed an index
 * that passed the stream fingerprint but whose block lengths disagreed with
 * the decoded blocks (an index made for another stream): that call decoded
 * the stream again after an index scan, so its output is still correct. */
int zfp_hip_last_stale_index(void);

/*
 * Device scratch: calls borrow a context (HIP stream + reusable buffers) from
 * a process-wide pool, so scratch is bounded by the peak number of concurrent
 * calls.  zfp_hip_scratch_bytes() reports what idle contexts hold;
 * zfp_hip_release_scratch() frees them (returns how many were freed).
 */
size_t zfp_hip_scratch_bytes(void);
int zfp_hip_release_scratch(void);

#ifdef __cplusplus
}
#endif

#endif
