// Host shim: what a job asks for (Plan) and where its stream and field image sit.
#pragma once

#include "host_ctx.h"
#include "kernels_n.h"
#include "launch.h"

using namespace zfp_amd;

// job analysis
struct Plan {
  int dims = 0;
  int type = 0;      // zfp_type: 1 int32, 2 int64, 3 float, 4 double
  size_t es = 0;     // bytes per value
  bool dbl = false;  // double (the f64 float kernels)
  Geometry g{};
  CodecParams cp{};
  bool fixed = false;        // every block exactly maxbits bits
  bool vec = false;          // 16-byte row loads/stores possible
  uint32_t bound_bits = 0;   // max bits a block writes (excl. padding)
  uint32_t max_len = 0;      // max block length incl. padding
  int64_t span_lo = 0, span_hi = 0;  // element offsets touched by the box
  uint32_t per_wave = 0;     // blocks a wave codes (64: 1D-3D, 16: 4D): the launch and block index layout
  uint64_t nwaves = 0;       // waves that cover the blocks
  size_t span_bytes() const { return (size_t)(span_hi - span_lo + 1) * es; }
};

static int plan_job(const zfp_hip_job* j, const void* field_base, Plan& p)
{
  if (!j)
    return fail("null job");
  if (j->type < 1 || j->type > 4)
    return fail("zfp_hip: scalar type %d not supported", j->type);
  if (j->dims < 1 || j->dims > 4)
    return fail("zfp_hip: %dD fields are not supported", j->dims);
  p.dims = j->dims;
  p.type = j->type;
  p.dbl = j->type == 4;
  p.es = (j->type == 2 || j->type == 4) ? 8 : 4;
  p.cp.minbits = j->minbits;
  p.cp.maxbits = j->maxbits;
  p.cp.maxprec = j->maxprec;
  p.cp.minexp = j->minexp;
  if (p.cp.maxprec == 0 || p.cp.maxprec > 64)
    return fail("zfp_hip: invalid maxprec %u", p.cp.maxprec);
  p.g.nblocks = 1;
  p.span_lo = p.span_hi = 0;
  for (int a = 0; a < 4; a++) {
    p.g.n[a] = a < p.dims ? j->n[a] : 1;
    p.g.s[a] = a < p.dims ? j->s[a] : 0;
    p.g.f[a] = a < p.dims ? j->f[a] : 0;
    uint64_t e = a < p.dims ? j->e[a] : 1;
    uint64_t nb = (a < p.dims) ? (e > p.g.f[a] ? (e - p.g.f[a] + 3) / 4 : 0) : 1;
    if (a < p.dims && e > p.g.n[a])
      return fail("zfp_hip: chunk end %llu exceeds field extent %llu on axis %d", (unsigned long long)e,
                  (unsigned long long)p.g.n[a], a);
    if (nb > 0xffffffffull)
      return fail("zfp_hip: too many blocks along axis %d", a);
    p.g.nb[a] = (uint32_t)nb;
    p.g.nblocks *= nb;
    if (a < p.dims && e > p.g.f[a]) {
      int64_t d0 = (int64_t)p.g.f[a] * p.g.s[a];
      // a block reads whole 4-blocks past a chunk end that is not block aligned
      // (up to the field edge, compress.c:127-133): the span covers them
      const uint64_t eb = std::min<uint64_t>(p.g.n[a], p.g.f[a] + 4 * nb);
      int64_t d1 = (int64_t)(eb - 1) * p.g.s[a];
      p.span_lo += std::min(d0, d1);
      p.span_hi += std::max(d0, d1);
    }
  }
  if (p.g.nblocks >> 32)
    return fail("zfp_hip: %llu blocks in one call (at most 2^32 - 1)", (unsigned long long)p.g.nblocks);
  p.per_wave = p.dims == 4 ? kBlocks4PerWave : 64u;
  p.nwaves = (p.g.nblocks + p.per_wave - 1) / p.per_wave;
  for (int a = 0; a < 3; a++)
    p.g.dv[a] = make_fastdiv(p.g.nb[a]);
  const bool integer = p.type <= 2;
  const int ebits = integer ? 0 : p.dbl ? 11 : 8, pbits = p.es == 8 ? 6 : 5, intprec = p.es == 8 ? 64 : 32;
  const bool rev = p.cp.minexp < kMinExp;
  // header bits (zfp.c block bounds): integers have none in lossy modes
  const uint32_t hdr = integer ? (rev ? pbits : 0) : (rev ? 2 + ebits + pbits : 1 + ebits);
  const uint64_t bvals = 1ull << (2 * p.dims);  // values per block
  uint64_t body = hdr + (bvals - 1) + bvals * std::min<uint32_t>(p.cp.maxprec, intprec);
  uint64_t bound = body;
  if (p.cp.maxbits >= hdr)
    bound = std::min<uint64_t>(bound, p.cp.maxbits);
  p.bound_bits = (uint32_t)bound;
  p.max_len = std::max<uint32_t>(p.bound_bits, p.cp.minbits);
  p.fixed = !rev && p.cp.minbits == p.cp.maxbits && p.cp.maxbits >= (uint32_t)(integer ? 1 : 1 + ebits);
  const size_t es = p.es;
  p.vec = p.g.s[0] == 1 && (p.g.s[1] % 4) == 0 && (p.g.s[2] % 4) == 0 && (p.g.f[0] % 4) == 0 &&
          (p.dims < 4 || (p.g.s[3] % 4) == 0) && ((uintptr_t)field_base % (4 * es)) == 0;
  if (!p.fixed && p.max_len > 0xffff)
    return fail("zfp_hip: block length bound %u bits exceeds the block index (16-bit lengths)", p.max_len);
  return 1;
}

// Where a call's first bit sits in the caller's stream: bit g0 of word W0, with
// `avail` words from there to the stream's capacity.
struct StreamPos {
  uint64_t W0;
  uint32_t g0;
  uint64_t avail;
  StreamPos(uint64_t bit_offset, uint64_t capacity_words)
      : W0(bit_offset >> 6), g0((uint32_t)(bit_offset & 63)), avail(capacity_words > W0 ? capacity_words - W0 : 0)
  {
  }
  // words a decoder is given for `bits` bits: one of lookahead, cut at the capacity
  uint64_t decode_words(uint64_t bits) const { return std::min<uint64_t>((g0 + bits + 63) / 64 + 1, avail); }
};

// Device image of a host field's span in the context's scratch: *d_img is the
// device pointer that corresponds to the host's field_base.
static int field_image(Ctx* c, const Plan& p, char** d_img)
{
  if (!ensure(c->field, p.span_bytes()))
    return 0;
  *d_img = (char*)c->field.p - p.span_lo * (int64_t)p.es;
  return 1;
}

static size_t slot_words_odd(uint32_t bits)
{
  return slot_words_for(bits) | 1;  // odd stride: fewer LDS bank collisions between lanes
}
