// Host shim: an index and the stream it describes -- fingerprint, publication,
// slab views and the match test.
#pragma once

#include "host_plan.h"

// Fingerprint of the stream bits [start_bit, start_bit + total_bits): a hash
// of the bit count and of 16 words spread evenly over the range (the first
// and last masked to the range).  Two streams of one field and mode whose
// block lengths differ anywhere differ in the words after that block, so an
// index is not used for a stream it does not describe (a stream that matches
// in every sampled word and in length has, in practice, the same block
// offsets).  Host streams are read in place; device streams through a small
// gather kernel.
constexpr int kFpWords = 16;

static __global__ void fp_gather(const uint64_t* __restrict__ w, uint64_t W0, uint64_t n, uint64_t* __restrict__ out)
{
  const uint32_t i = threadIdx.x;
  if (i < kFpWords)
    out[i] = w[W0 + (n - 1) * i / (kFpWords - 1)];
}

static uint64_t fp_mix(uint64_t h, uint64_t v)
{
  h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
  return h * 0xff51afd7ed558ccdull;
}

static int stream_fingerprint(Ctx* c, const uint64_t* words, bool dev, uint64_t start_bit, uint64_t total_bits,
                              uint64_t* fp)
{
  const uint64_t W0 = start_bit >> 6, end = start_bit + total_bits;
  const uint64_t n = total_bits ? ((end + 63) >> 6) - W0 : 1;
  uint64_t v[kFpWords];
  if (dev) {
    if (!ensure(c->fpbuf, kFpWords * 8))
      return 0;
    hipLaunchKernelGGL(fp_gather, dim3(1), dim3(64), 0, c->stream, words, W0, n, (uint64_t*)c->fpbuf.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(v, c->fpbuf.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  } else {
    for (int i = 0; i < kFpWords; i++)
      v[i] = words[W0 + (n - 1) * (uint64_t)i / (kFpWords - 1)];
  }
  uint64_t h = fp_mix(0x7a6670ull, total_bits);
  for (int i = 0; i < kFpWords; i++) {
    const uint64_t wi = W0 + (n - 1) * (uint64_t)i / (kFpWords - 1);
    uint64_t m = ~0ull;
    if (wi == W0)
      m &= ~0ull << (start_bit & 63);
    if (total_bits && wi == ((end - 1) >> 6) && (end & 63))
      m &= (1ull << (end & 63)) - 1;
    if (!total_bits)
      m = 0;
    h = fp_mix(h, v[i] & m);
  }
  *fp = h;
  return 1;
}

// the codec settings and layout an index is made for
static void index_stamp(zfp_hip_index* x, const Plan& p)
{
  x->minbits = p.cp.minbits;
  x->maxbits = p.cp.maxbits;
  x->maxprec = p.cp.maxprec;
  x->minexp = p.cp.minexp;
  x->type = p.type;
  x->dims = p.dims;
}

static void index_layout(IndexView* x, const Ctx* c, const Plan& p)
{
  x->device = c->device;
  x->nblocks = p.g.nblocks;
  x->nwaves = p.nwaves;
  x->per_wave = p.per_wave;
}

// An encode is about to fill `x`: room for the job's layout; the index
// describes no stream until index_publish.
static int index_begin(zfp_hip_index* x, const Ctx* c, const Plan& p)
{
  x->start_bit = ~0ull;
  if (!index_reserve(x, p.g.nblocks, p.nwaves))
    return 0;
  index_layout(x, c, p);
  return 1;
}

// `x` now holds the lengths and bases of the `total_bits` bits at `bit_offset`
// of `words`: from here on it is used for that stream (index_matches).
static int index_publish(Ctx* c, zfp_hip_index* x, const Plan& p, const uint64_t* words, bool dev_stream,
                         uint64_t bit_offset, uint64_t total_bits)
{
  x->total_bits = total_bits;
  index_stamp(x, p);
  if (!stream_fingerprint(c, words, dev_stream, bit_offset, total_bits, &x->fp))
    return 0;
  x->start_bit = bit_offset;
  return 1;
}

// The part of `x` that covers the blocks of slab plan `p` from `first_block`
// (a whole number of waves) on; the bases stay relative to x's first block.
static IndexView index_view(const zfp_hip_index* x, uint64_t first_block, const Plan& p)
{
  IndexView v = *x;
  v.nblocks = p.g.nblocks;
  v.nwaves = p.nwaves;
  v.d_len += first_block;
  v.d_base += first_block / p.per_wave;
  return v;
}

// the index was made for this stream: same codec settings, layout, bit offset
// and device, and the stream's fingerprint over the index's bit count agrees
static bool index_matches(Ctx* c, const zfp_hip_index* x, const Plan& p, const uint64_t* words, bool dev_stream,
                          uint64_t capacity_words, uint64_t bit_offset)
{
  if (!(x && x->d_len && x->nblocks == p.g.nblocks && x->start_bit == bit_offset && x->device == c->device &&
        x->per_wave == p.per_wave && x->minbits == p.cp.minbits &&
        x->maxbits == p.cp.maxbits && x->maxprec == p.cp.maxprec && x->minexp == p.cp.minexp && x->type == p.type &&
        x->dims == p.dims))
    return false;
  if (((bit_offset + x->total_bits + 63) >> 6) > capacity_words)
    return false;
  uint64_t fp = 0;
  if (!stream_fingerprint(c, words, dev_stream, bit_offset, x->total_bits, &fp)) {
    (void)hipGetLastError();
    return false;
  }
  return fp == x->fp;
}
