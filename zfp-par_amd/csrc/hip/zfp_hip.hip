// libzfp_hip.so -- MI355X codec library behind include/zfp_hip.h.
//
// Host side of the C-ABI: validates a job, works out where the field and the
// stream live (host or device), stages host buffers through the device scratch
// of a context leased from a process-wide pool for the call (its own HIP
// stream), picks a kernel path and launches it.
//
//   fixed rate, block size a multiple of 64 bits  -> encode3_aligned (+ one
//        funnel-shift pass when the stream offset is not word aligned)
//   everything else (variable rate, odd block sizes) -> encode3_general with
//        decoupled look-back, then fixup_zero/fixup_or for words shared by waves
//   decode: decode3 (fixed-rate offsets analytic, variable rate from the index)
//   4D: encode4 / decode4 (one block per quad of lanes, 16 blocks per wave),
//        every mode through the packing path of encode3_general
//
// One translation unit: this file holds the extern "C" surface, the host-only
// headers below the rest, each building on the ones before it.
#include <atomic>

#include "host_error.h"        // the per-thread error message, HIP_TRY
#include "host_index.h"        // zfp_hip_index and its device storage
#include "host_ctx.h"          // contexts, their pool, the per-call lease, pinned staging
#include "host_call.h"         // how a call opens, the index check word, the stale-index retries
#include "host_plan.h"         // Plan: what a job asks for
#include "host_index_match.h"  // an index and the stream it describes
#include "host_launch.h"       // encode and decode launchers
#include "host_scan.h"         // index scan of a stream without an index
#include "host_pipeline.h"     // host <-> device box copies, the slab pipeline
#include "host_rows.h"         // rows of a strided host array <-> a packed image (no HIP call)
#include "host_region.h"       // region decode, and the host pieces every region call shares
#include "host_region_enc.h"   // region encode: validation, source image, launch, copy-back
#include "host_boxes.h"        // batched region decode: validation, the region table, launch, copy-out
#include "host_boxes_enc.h"    // batched region encode: validation, disjointness, sources, launch, copy-back

// ---------------------------------------------------------------------------
// How every entry point that uses the device begins: the job's plan, the
// entry's own pointer arguments (`null_arg` names the one that is null), a
// device to run on, a context, and fresh per-call timing.  `index_call`: the
// entry works on a block index, which only variable-rate streams have.
static int begin_call(CtxLease& lease, const char* who, const zfp_hip_job* job, const void* field_base,
                      const char* null_arg, bool index_call, int device, Plan& p)
{
  t_timing = Timing{};  // a call refused below is still this thread's most recent call
  if (!plan_job(job, field_base, p))
    return 0;
  if (null_arg)
    return fail("%s: null %s", who, null_arg);
  if (index_call && p.fixed)
    return fail("%s: fixed-rate streams need no index", who);
  return open_call(lease, who, device);
}

extern "C" {

int zfp_hip_device_count(void)
{
  // asked by every entry point: queried once (7 us a call), devices do not come and go
  static std::atomic<int> cached{-1};
  int n = cached.load(std::memory_order_relaxed);
  if (n >= 0)
    return n;
  n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  cached.store(n, std::memory_order_relaxed);
  return n;
}

const char* zfp_hip_last_error(void) { return g_err.c_str(); }

int zfp_hip_is_device_ptr(const void* p)
{
  static int ndev = -1;  // benign race: every thread computes the same value
  if (ndev < 0)
    ndev = zfp_hip_device_count();
  return ndev > 0 && is_device_ptr(p) ? 1 : 0;
}

int zfp_hip_memcpy(void* dst, const void* src, size_t bytes)
{
  if (hipMemcpy(dst, src, bytes, hipMemcpyDefault) != hipSuccess)
    return fail("hipMemcpy(%zu) failed", bytes);
  return 1;
}

int zfp_hip_compress(const zfp_hip_job* job, const void* field_base, uint64_t* words, uint64_t capacity_words,
                     uint64_t bit_offset, uint64_t head_word, int device, zfp_hip_index* index, uint64_t* end_bit)
{
  Plan p;
  CtxLease lease;
  if (!begin_call(lease, "zfp_hip_compress", job, field_base,
                  !field_base || !words ? "field or stream pointer" : nullptr, false, device, p))
    return 0;
  Ctx* c = lease.c;
  const uint64_t W0 = bit_offset >> 6;
  const uint32_t g0 = (uint32_t)(bit_offset & 63);
  if (p.g.nblocks == 0) {
    *end_bit = bit_offset;
    return lease.done(1);
  }
  const uint64_t worst_bits = (uint64_t)g0 + p.g.nblocks * (uint64_t)(p.fixed ? p.cp.maxbits : p.max_len);
  const uint64_t worst_words = (worst_bits + 63) / 64 + 1;
  const bool dev_field = is_device_ptr(field_base);
  const bool dev_stream = is_device_ptr(words);
  if (p.fixed && W0 + (worst_bits + 63) / 64 > capacity_words)
    return fail("zfp_hip_compress: stream capacity %llu words < %llu needed", (unsigned long long)capacity_words,
                (unsigned long long)(W0 + (worst_bits + 63) / 64));
  if (!dev_field && !dev_stream && !getenv("ZFP_HIP_NO_PIPE")) {
    std::vector<Slab> sl;
    if (make_slabs(job, field_base, p, sl))
      return lease.done(timed_wall([&] {
        return by_type(p, [&](auto tag) {
          using S = std::remove_pointer_t<decltype(tag)>;
          return compress_slabs<S>(c, p, sl, field_base, words, capacity_words, bit_offset, head_word, index, end_bit);
        });
      }));
  }
  // stream
  const bool direct = dev_stream && W0 + worst_words <= capacity_words;
  c->one_pair = dev_field && direct && one_kernel_encode(p, g0);
  if (!c->one_pair)
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  // field
  const void* d_field = field_base;
  if (!dev_field) {
    char* d_img;
    if (!field_image(c, p, &d_img) || !copy_box(c, p, (void*)field_base, d_img, p.es, false))
      return 0;
    d_field = d_img;
  }
  if (p.fixed)
    index = nullptr;
  if (index && !index_begin(index, c, p))
    return 0;
  uint64_t* d_out;
  if (direct) {
    d_out = words + W0;
  } else {
    if (!ensure(c->words, worst_words * 8))
      return 0;
    d_out = (uint64_t*)c->words.p;
  }
  uint64_t total = 0;
  Head head;
  head.val = head_word;
  int ok = by_type(p, [&](auto tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    return launch_encode<S>(c, p, (const S*)d_field, d_out, g0, head, index, &total);
  });
  if (!ok)
    return 0;
  // one_kernel_encode predicted the path before the launch; launch_encode says which it took
  if (c->one_pair && !c->single_kernel)
    return fail("zfp_hip_compress: internal: the encode queued more than one kernel on the two-event path");
  const uint64_t end = bit_offset + total;
  const uint64_t nwords = (g0 + total + 63) / 64;
  if (W0 + nwords > capacity_words)
    return fail("zfp_hip_compress: compressed stream (%llu words) exceeds capacity %llu",
                (unsigned long long)(W0 + nwords), (unsigned long long)capacity_words);
  char* staged = nullptr;  // small host stream: through pinned memory, copied out after the synchronize
  if (!direct) {
    hipMemcpyKind kind = dev_stream ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    staged = dev_stream ? nullptr : pin_take(c, nwords * 8);
    HIP_TRY(hipMemcpyAsync(staged ? (void*)staged : (void*)(words + W0), d_out, nwords * 8, kind, c->stream));
  }
  if (!c->one_pair)
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (staged)
    memcpy(words + W0, staged, nwords * 8);
  record_timing(c);
  if (index && !index_publish(c, index, p, words, dev_stream, bit_offset, total))
    return 0;
  *end_bit = end;
  return lease.done(1);
}

// One decompression with the given index (nullptr: the stream is scanned;
// plain_scan: with ordinary scan passes only).
// *stale: the decoded block lengths disagreed with the index -- a caller's
// index that had passed index_matches (it belongs to another stream) or the
// scan's own; the output is garbage and the caller decodes again with a
// (plain) scan.  *scanned: the index was the scan's.
static int decompress_once(Ctx* c, const Plan& p, const zfp_hip_job* job, void* field_base, const uint64_t* words,
                           uint64_t capacity_words, uint64_t bit_offset, const zfp_hip_index* index,
                           uint64_t* end_bit, bool plain_scan, bool* stale, bool* scanned)
{
  const StreamPos at(bit_offset, capacity_words);
  const uint64_t W0 = at.W0;
  const uint32_t g0 = at.g0;
  const bool dev_field = is_device_ptr(field_base);
  const bool dev_stream = is_device_ptr(words);
  // a variable-rate stream without a matching index (made by another
  // process, another library, or for another stream or position) is scanned
  const bool have_index = !p.fixed && index_matches(c, index, p, words, dev_stream, capacity_words, bit_offset);
  const bool scan = !p.fixed && !have_index;
  *scanned = scan;
  CheckWord chk{c};  // (a variable-rate index is verified by the decode kernels: host_call.h)
  if (!chk.arm(p.fixed))
    return 0;
  const uint64_t nwords = at.decode_words(p.fixed      ? p.g.nblocks * (uint64_t)p.cp.maxbits
                                          : have_index ? index->total_bits
                                                       : p.g.nblocks * (uint64_t)p.max_len);
  if ((p.fixed || have_index) && !dev_field && !dev_stream && !getenv("ZFP_HIP_NO_PIPE")) {
    std::vector<Slab> sl;
    if (make_slabs(job, field_base, p, sl)) {
      const int ok = timed_wall([&] {
        return by_type(p, [&](auto tag) {
          using S = std::remove_pointer_t<decltype(tag)>;
          return decompress_slabs<S>(c, p, sl, field_base, words, capacity_words, bit_offset, index, end_bit);
        });
      });
      return ok ? chk.verdict(stale) : 0;
    }
  }
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  const uint64_t* d_in = words + W0;
  if (!dev_stream) {
    if (!ensure(c->words, nwords * 8 + 8))
      return 0;
    if (!h2d(c, c->words.p, words + W0, nwords * 8, c->stream))
      return 0;
    d_in = (const uint64_t*)c->words.p;
  }
  if (scan) {
    if (!scan_index(c, p, d_in, nwords, g0, &c->scan_index, plain_scan))
      return 0;
    c->scan_index.start_bit = bit_offset;
    index = &c->scan_index;
  }
  const uint64_t total = p.fixed ? p.g.nblocks * (uint64_t)p.cp.maxbits : index->total_bits;
  void* d_field = field_base;
  char* d_img = nullptr;
  if (!dev_field) {
    if (!field_image(c, p, &d_img))
      return 0;
    d_field = d_img;
  }
  int ok = by_type(p, [&](auto tag) {
    using S = std::remove_pointer_t<decltype(tag)>;
    return launch_decode<S>(c, p, (S*)d_field, d_in, nwords, g0, index);
  });
  if (!ok)
    return 0;
  if (!chk.queue())
    return 0;
  if (!dev_field && !copy_box(c, p, field_base, d_img, p.es, true))
    return 0;
  HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  record_timing(c);
  *end_bit = bit_offset + total;
  return chk.verdict(stale);
}

int zfp_hip_decompress(const zfp_hip_job* job, void* field_base, const uint64_t* words, uint64_t capacity_words,
                       uint64_t bit_offset, int device, const zfp_hip_index* index, uint64_t* end_bit)
{
  Plan p;
  CtxLease lease;
  if (!begin_call(lease, "zfp_hip_decompress", job, field_base,
                  !field_base || !words ? "field or stream pointer" : nullptr, false, device, p))
    return 0;
  Ctx* c = lease.c;
  if (p.g.nblocks == 0) {
    *end_bit = bit_offset;
    return lease.done(1);
  }
  const int ok = with_stale_retry("zfp_hip_decompress", index,
                                  [&](const zfp_hip_index* x, bool plain, bool* stale, bool* scanned) {
                                    return decompress_once(c, p, job, field_base, words, capacity_words, bit_offset, x,
                                                           end_bit, plain, stale, scanned);
                                  });
  return lease.done(ok);
}

// (The region entries do not go through begin_call: the job's strides are
// unused, and everything is validated before the first GPU call, the device
// count included.)
int zfp_hip_decompress_region(const zfp_hip_job* job, const uint64_t lo[4], const uint64_t hi[4], void* dst,
                              const int64_t dst_stride[4], const uint64_t* words, uint64_t capacity_words,
                              uint64_t bit_offset, int device, const zfp_hip_index* index, uint64_t* blocks_read)
{
  const char* who = "zfp_hip_decompress_region";
  Plan p;
  RegionGeom rg;
  CtxLease lease;
  t_timing = Timing{};  // (as begin_call: a region refused before open_call reports no scan, no timing)
  if (!plan_region(job, lo, hi, dst, dst_stride, words, p, rg) || !open_call(lease, who, device))
    return 0;
  const int ok = with_stale_retry(who, index, [&](const zfp_hip_index* x, bool plain, bool* stale, bool* scanned) {
    return region_once(lease.c, p, rg, dst, dst_stride,
                       DecodeTry{words, capacity_words, bit_offset, x, plain, stale, scanned});
  });
  if (ok && blocks_read)
    *blocks_read = rg.nrblocks;
  return lease.done(ok);
}

int zfp_hip_decompress_regions(const zfp_hip_job* job, const zfp_hip_region* regions, uint64_t nregions,
                               const uint64_t* words, uint64_t capacity_words, uint64_t bit_offset, int device,
                               const zfp_hip_index* index, uint64_t* blocks_read)
{
  const char* who = "zfp_hip_decompress_regions";
  Plan p;
  BoxesPlan bp;
  std::vector<BoxRecord> rec;  // (outlives the lease: it may have to wait for the table's copy)
  t_timing = Timing{};
  if (!plan_regions(job, regions, nregions, words, p, bp))
    return 0;
  if (nregions == 0) {
    if (blocks_read)
      *blocks_read = 0;
    return 1;
  }
  CtxLease lease;
  if (!open_call(lease, who, device))
    return 0;
  // (a stale index repeats the whole batch)
  const int ok = with_stale_retry(who, index, [&](const zfp_hip_index* x, bool plain, bool* stale, bool* scanned) {
    return regions_once(lease.c, p, bp, rec, regions,
                        DecodeTry{words, capacity_words, bit_offset, x, plain, stale, scanned});
  });
  if (ok && blocks_read)
    *blocks_read = bp.blocks;
  return lease.done(ok);
}

int zfp_hip_compress_region(const zfp_hip_job* job, const uint64_t lo[4], const uint64_t hi[4], const void* src,
                            const int64_t src_stride[4], uint64_t* words, uint64_t capacity_words,
                            uint64_t bit_offset, int device, uint64_t* blocks_written)
{
  Plan p;
  RegionGeom rg;
  CtxLease lease;
  t_timing = Timing{};
  if (!plan_region_enc(job, lo, hi, src, src_stride, words, capacity_words, bit_offset, p, rg) ||
      !open_call(lease, "zfp_hip_compress_region", device))
    return 0;
  const int ok = region_enc_once(lease.c, p, rg, src, src_stride, words, capacity_words, bit_offset);
  if (ok && blocks_written)
    *blocks_written = rg.nrblocks;
  return lease.done(ok);
}

int zfp_hip_compress_regions(const zfp_hip_job* job, const zfp_hip_src_region* regions, uint64_t nregions,
                             uint64_t* words, uint64_t capacity_words, uint64_t bit_offset, int device,
                             uint64_t* blocks_written)
{
  const char* who = "zfp_hip_compress_regions";
  Plan p;
  BoxesPlan bp;
  std::vector<BoxRecord> rec;          // (these outlive the lease: they may have to wait for their copies)
  std::vector<std::vector<char>> tmp;  // packed rows of host sources
  t_timing = Timing{};
  if (!plan_regions_enc(job, regions, nregions, words, capacity_words, bit_offset, p, bp))
    return 0;
  if (nregions == 0) {
    if (blocks_written)
      *blocks_written = 0;
    return 1;
  }
  CtxLease lease;
  if (!open_call(lease, who, device))
    return 0;
  const int ok = regions_enc_once(lease.c, p, bp, rec, tmp, regions, words, capacity_words, bit_offset);
  if (ok && blocks_written)
    *blocks_written = bp.blocks;
  return lease.done(ok);
}

int zfp_hip_index_build(const zfp_hip_job* job, const uint64_t* words, uint64_t capacity_words, uint64_t bit_offset,
                        int device, zfp_hip_index* index)
{
  Plan p;
  CtxLease lease;
  if (!begin_call(lease, "zfp_hip_index_build", job, nullptr, !index ? "index" : !words ? "stream" : nullptr, true,
                  device, p))
    return 0;
  Ctx* c = lease.c;
  const bool dev_stream = is_device_ptr(words);
  if (p.g.nblocks == 0) {  // nothing to scan (and nothing queued)
    index->nblocks = 0;
    index->nwaves = 0;
    index->total_bits = 0;
  } else {
    const StreamPos at(bit_offset, capacity_words);
    const uint64_t nwords = at.decode_words(p.g.nblocks * (uint64_t)p.max_len);
    const uint64_t* d_in = words + at.W0;
    if (!dev_stream) {
      if (!ensure(c->words, nwords * 8 + 8))
        return 0;
      HIP_TRY(hipMemcpyAsync(c->words.p, words + at.W0, nwords * 8, hipMemcpyHostToDevice, c->stream));
      d_in = (const uint64_t*)c->words.p;
    }
    if (!scan_index(c, p, d_in, nwords, at.g0, index))
      return 0;
  }
  return lease.done(index_publish(c, index, p, words, dev_stream, bit_offset, index->total_bits));
}

int zfp_hip_index_set_offsets(zfp_hip_index* index, const zfp_hip_job* job, const uint64_t* words,
                              uint64_t capacity_words, uint64_t bit_offset, const uint64_t* offsets, uint64_t count,
                              int device)
{
  Plan p;
  std::vector<uint16_t> len;  // (outlive the lease: it may have to wait for their copies)
  std::vector<uint64_t> base;
  CtxLease lease;
  if (!begin_call(lease, "zfp_hip_index_set_offsets", job, nullptr,
                  !index || !offsets ? "index or offsets" : !words ? "stream" : nullptr, true, device, p))
    return 0;
  Ctx* c = lease.c;
  if (p.g.nblocks != count)
    return fail("zfp_hip_index_set_offsets: %llu offsets for %llu blocks", (unsigned long long)count,
                (unsigned long long)p.g.nblocks);
  const uint32_t per = p.per_wave;
  const uint64_t nwaves = p.nwaves;
  len.resize(count);
  base.resize(nwaves);
  for (uint64_t b = 0; b < count; b++) {
    if (offsets[b + 1] < offsets[b] || offsets[b + 1] - offsets[b] > 0xffffu)
      return fail("zfp_hip_index_set_offsets: block %llu has no valid length", (unsigned long long)b);
    len[b] = (uint16_t)(offsets[b + 1] - offsets[b]);
  }
  for (uint64_t w = 0; w < nwaves; w++)
    base[w] = offsets[w * per] - offsets[0];
  const uint64_t total = offsets[count] - offsets[0];
  if (((bit_offset + total + 63) >> 6) > capacity_words)
    return fail("zfp_hip_index_set_offsets: the blocks run past the stream's %llu words",
                (unsigned long long)capacity_words);
  if (!index_begin(index, c, p))
    return 0;
  if (count && !h2d(c, index->d_len, len.data(), count * 2, c->stream))
    return 0;
  if (nwaves && !h2d(c, index->d_base, base.data(), nwaves * 8, c->stream))
    return 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return lease.done(index_publish(c, index, p, words, is_device_ptr(words), bit_offset, total));
}

zfp_hip_index* zfp_hip_index_create(void) { return new zfp_hip_index; }

void zfp_hip_index_free(zfp_hip_index* index)
{
  if (!index)
    return;
  index_release(index);
  delete index;
}

uint64_t zfp_hip_index_blocks(const zfp_hip_index* index) { return index ? index->nblocks : 0; }

// exported index: a 10-word head (tag, layout, bit count, fingerprint, codec
// settings), the per-block lengths, the per-wave bases
constexpr size_t kIndexHead = 80;
constexpr uint64_t kIndexTag = 0x337a6678646e69ull;  // "indxfz3"

size_t zfp_hip_index_export(const zfp_hip_index* index, void* buffer, size_t capacity)
{
  if (!index)
    return 0;
  size_t need = kIndexHead + index->nblocks * 2 + index->nwaves * 8;
  if (!buffer)
    return need;
  if (capacity < need)
    return 0;
  uint64_t* h = (uint64_t*)buffer;
  h[0] = kIndexTag;
  h[1] = index->nblocks;
  h[2] = index->nwaves;
  h[3] = index->total_bits;
  h[4] = index->per_wave;
  h[5] = index->start_bit;
  h[6] = index->fp;
  h[7] = ((uint64_t)index->maxbits << 32) | index->minbits;
  h[8] = ((uint64_t)(uint32_t)index->minexp << 32) | index->maxprec;
  h[9] = ((uint64_t)(uint32_t)index->dims << 32) | (uint32_t)index->type;
  char* q = (char*)buffer + kIndexHead;
  if (index->nblocks && hipMemcpy(q, index->d_len, index->nblocks * 2, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  q += index->nblocks * 2;
  if (index->nwaves && hipMemcpy(q, index->d_base, index->nwaves * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  return need;
}

zfp_hip_index* zfp_hip_index_import(const void* buffer, size_t bytes)
{
  if (!buffer || bytes < kIndexHead)
    return nullptr;
  const uint64_t* h = (const uint64_t*)buffer;
  if (h[0] != kIndexTag || h[1] > (1ull << 32) || h[2] > h[1] || bytes < kIndexHead + h[1] * 2 + h[2] * 8)
    return nullptr;
  zfp_hip_index* x = new zfp_hip_index;
  x->nblocks = h[1];
  x->nwaves = h[2];
  x->total_bits = h[3];
  x->per_wave = (uint32_t)h[4];
  x->start_bit = h[5];
  x->fp = h[6];
  x->minbits = (uint32_t)h[7];
  x->maxbits = (uint32_t)(h[7] >> 32);
  x->maxprec = (uint32_t)h[8];
  x->minexp = (int32_t)(uint32_t)(h[8] >> 32);
  x->type = (int32_t)(uint32_t)h[9];
  x->dims = (int32_t)(uint32_t)(h[9] >> 32);
  (void)hipGetDevice(&x->device);
  const char* q = (const char*)buffer + kIndexHead;
  if ((x->nblocks && hipMalloc(&x->d_len, x->nblocks * 2) != hipSuccess) ||
      (x->nwaves && hipMalloc(&x->d_base, x->nwaves * 8) != hipSuccess)) {
    zfp_hip_index_free(x);
    return nullptr;
  }
  x->cap_blocks = x->nblocks;
  x->cap_waves = x->nwaves;
  if (x->nblocks)
    (void)hipMemcpy(x->d_len, q, x->nblocks * 2, hipMemcpyHostToDevice);
  if (x->nwaves)
    (void)hipMemcpy(x->d_base, q + x->nblocks * 2, x->nwaves * 8, hipMemcpyHostToDevice);
  return x;
}

uint64_t zfp_hip_index_offsets(const zfp_hip_index* index, uint64_t* offsets, uint64_t count)
{
  if (!index)
    return 0;
  const uint64_t n = index->nblocks;
  if (!offsets)
    return n + 1;
  if (count < n + 1)
    return fail("zfp_hip_index_offsets: %llu entries needed", (unsigned long long)(n + 1));
  std::vector<uint16_t> len(n);
  if (n && hipMemcpy(len.data(), index->d_len, n * 2, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("zfp_hip_index_offsets: copy of the block lengths failed");
  uint64_t p = 0;
  for (uint64_t b = 0; b < n; b++) {
    offsets[b] = p;
    p += len[b];
  }
  offsets[n] = p;
  return n + 1;
}

int zfp_hip_last_timing(double* kernel_ms, double* total_ms)
{
  if (!t_timing.timed)
    return 0;
  if (kernel_ms) *kernel_ms = t_timing.kernel_ms;
  if (total_ms) *total_ms = t_timing.total_ms;
  return 1;
}

int zfp_hip_last_stale_index(void) { return t_timing.stale_index ? 1 : 0; }

int zfp_hip_last_scan(double* scan_ms, int* passes)
{
  if (!t_timing.scan_passes)
    return 0;
  if (scan_ms) *scan_ms = t_timing.scan_ms;
  if (passes) *passes = t_timing.scan_passes;
  return 1;
}

size_t zfp_hip_scratch_bytes(void)
{
  std::lock_guard<std::mutex> lk(g_pool_mu);
  size_t b = 0;
  for (Ctx* c : g_idle) {
    for (const Scratch* s : {&c->field, &c->words, &c->status, &c->partials, &c->misc, &c->ovf, &c->scan_bm, &c->scan_seg,
                             &c->scan_tiles, &c->scan_pos, &c->boxes})
      b += s->bytes;
    b += c->scan_index.cap_blocks * 2 + c->scan_index.cap_waves * 8;
  }
  return b;
}

int zfp_hip_release_scratch(void)
{
  std::vector<Ctx*> idle;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    idle.swap(g_idle);
  }
  for (Ctx* c : idle)
    destroy_ctx(c);
  return (int)idle.size();
}

}  // extern "C"
