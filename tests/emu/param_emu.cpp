// Host run of the device block codecs against the C oracle over codec
// parameters given on stdin (or in the file named by argv[1]); fed from
// tests/params.py by tests/test_emu_params.py.  Lines:
//
//   e <type> <exponent> ...                     ladder exponents of a type (3 float, 4 double)
//   p <type> <dims> <minbits> <maxbits> <maxprec> <minexp>
//
// Every `p` line runs, over one ladder block per exponent of its type (largest
// magnitude exactly 2^e, the rest uniform below it, a few values at 2^(e-40)
// and at 0, mixed signs) and over blocks of +0, -0, NaN, one Inf, one denormal
// and +-max:
//   3D  encode_block3 / decode_block3 (block3.h), with the fixed-rate coder
//       <S, false, true> and the planes-32..63 coder and decoder under the
//       launchers' own rules (fixed_rate_coder_applies, kHiPlanesMaxPrec)
//   1D, 2D  encode_block_n / decode_block_n (blockn.h)
//   4D  the quad codec (block4.h) as four threads, as in quad_emu.cpp
// bit for bit against oz_compress / oz_decompress.  Encoder slots and decoder
// staging have the sizes the launchers give them (host_launch.h), as exact heap
// blocks: built with -fsanitize=address,undefined an out-of-slot access at an
// untried parameter is reported here, on the CPU.
#include <hip/hip_runtime.h>

#include <atomic>
#include <thread>

struct EmuTid {
  uint32_t x;
};
inline thread_local EmuTid threadIdx{0};

// generation barrier for the four lane threads of a quad
struct QuadBarrier {
  std::atomic<int> n{0};
  std::atomic<unsigned> gen{0};
  void wait()
  {
    const unsigned g = gen.load(std::memory_order_acquire);
    if (n.fetch_add(1, std::memory_order_acq_rel) == 3) {
      n.store(0, std::memory_order_relaxed);
      gen.fetch_add(1, std::memory_order_release);
    } else {
      while (gen.load(std::memory_order_acquire) == g)
        std::this_thread::yield();
    }
  }
};
inline QuadBarrier g_bar;
inline std::atomic<uint32_t> g_xchg[4];

inline int __builtin_amdgcn_mov_dpp(int x, int ctrl, int, int, bool)
{
  const uint32_t r = threadIdx.x & 3u;
  g_xchg[r].store((uint32_t)x, std::memory_order_relaxed);
  g_bar.wait();
  const int v = (int)g_xchg[(ctrl >> (2 * r)) & 3].load(std::memory_order_relaxed);
  g_bar.wait();
  return v;
}
inline int __builtin_amdgcn_update_dpp(int, int x, int ctrl, int, int, bool)
{
  return __builtin_amdgcn_mov_dpp(x, ctrl, 0, 0, false);
}
inline void __syncthreads() { g_bar.wait(); }

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <vector>
#include <fstream>
#include <iostream>

#include "block4.h"
#include "blockn.h"
using namespace zfp_amd;

extern "C" {
typedef struct { uint32_t minbits, maxbits, maxprec; int32_t minexp; } oz_params;
typedef struct { int32_t type, pad_; oz_params p; uint64_t n[4]; int64_t s[4]; uint64_t f[4]; uint64_t e[4]; } oz_job;
uint64_t oz_compress(const oz_job* j, const void* data, uint64_t* words, uint64_t bitpos);
uint64_t oz_decompress(const oz_job* j, void* data, const uint64_t* words, uint64_t bitpos);
}

// slot sizes of the kernel headers, restated (the kernels themselves are not compiled here):
// kernels3.h slot_dwords_for (aligned encoders) and kernels4.h slot_words4 (4D encoder)
static constexpr uint32_t slot_dwords_for(uint32_t lim) { return (lim + 95u) / 32u + 1u; }
static constexpr uint32_t slot_words4(uint32_t lim) { return ((((lim + 31u) >> 5) + 4u) / 2u) | 1u; }

template <typename S>
using Blocks = std::vector<std::vector<S>>;

// n values per block: the ladder, then the special blocks
template <typename S>
static Blocks<S> make_blocks(const std::vector<int>& exps, int n, uint64_t seed)
{
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  Blocks<S> out;
  const int few = n / 16 > 1 ? n / 16 : 1;
  for (int e : exps) {
    std::vector<S> b(n);
    for (int i = 0; i < n; i++)
      b[i] = (S)std::ldexp(u(rng), e);
    std::vector<int> pos(n);
    for (int i = 0; i < n; i++)
      pos[i] = i;
    for (int i = n - 1; i > 0; i--)
      std::swap(pos[i], pos[rng() % (uint64_t)(i + 1)]);
    for (int k = 0; k < few && 1 + k < n; k++)
      b[pos[1 + k]] = (S)std::ldexp((rng() & 1) ? 1.0 : -1.0, e - 40);
    for (int k = 0; k < few && 1 + few + k < n; k++)
      b[pos[1 + few + k]] = (S)0;
    b[pos[0]] = (S)std::ldexp((rng() & 1) ? 1.0 : -1.0, e);
    out.push_back(b);
  }
  using L = std::numeric_limits<S>;
  std::vector<S> b(n);
  out.push_back(std::vector<S>(n, (S)0.0));
  out.push_back(std::vector<S>(n, (S)-0.0));
  out.push_back(std::vector<S>(n, L::quiet_NaN()));
  for (int i = 0; i < n; i++)
    b[i] = (S)u(rng);
  b[n / 3] = L::infinity();
  out.push_back(b);
  out.push_back(std::vector<S>(n, L::denorm_min() * 5));
  for (int i = 0; i < n; i++)
    b[i] = (i & 1) ? -L::max() : L::max();
  out.push_back(b);
  return out;
}

// host_plan.h plan_job: the most bits a block codes (without padding)
template <typename S>
static uint32_t bound_bits(const CodecParams& cp, int dims)
{
  using T = Traits<S>;
  const bool rev = cp.minexp < kMinExp;
  const uint32_t hdr = rev ? 2 + T::kEbits + T::kPbits : 1 + T::kEbits;
  const uint64_t vals = 1ull << (2 * dims);
  uint64_t bound = hdr + (vals - 1) + vals * std::min<uint32_t>(cp.maxprec, T::kIntPrec);
  if (cp.maxbits >= hdr)
    bound = std::min<uint64_t>(bound, cp.maxbits);
  return (uint32_t)bound;
}

static bool same_bits(const uint64_t* a, const uint64_t* b, uint64_t len)
{
  for (uint64_t i = 0; i < (len + 63) / 64; i++) {
    const uint64_t m = (i == len / 64 && (len & 63)) ? ((1ull << (len & 63)) - 1) : ~0ull;
    if ((a[i] & m) != (b[i] & m))
      return false;
  }
  return true;
}

struct Tables {
  std::vector<uint32_t> sq = std::vector<uint32_t>(256);
  std::vector<uint32_t> dbl = std::vector<uint32_t>(256);
  Tables()
  {
    for (int b = 0; b < 256; b++)
      sq[b] = squeeze_entry(b), dbl[b] = dbl_entry(b);
  }
};

// An encoder slot as encode3_general lays it out: swp words, preceded by the
// neighbouring lane's slot (a write at bit 0 ORs zero into the dword before).
struct Slot {
  std::vector<uint64_t> mem;
  uint32_t swp;
  explicit Slot(uint32_t bound) : swp((uint32_t)slot_words_for(bound) | 1u) { mem.assign(swp + 1, 0); }
  uint64_t* base() { return mem.data() + 1; }
  OrSlot os() { return OrSlot{base(), 2 * swp - 1}; }
  bool neighbour_clean() const { return mem[0] == 0; }
};

struct Oracle {
  oz_job j{};
  std::vector<uint64_t> w;
  uint64_t end = 0, dend = 0;
  template <typename S>
  void run(int type, int dims, const CodecParams& cp, const std::vector<S>& blk, std::vector<S>& dec)
  {
    j = oz_job{};
    j.type = type;
    j.p = {cp.minbits, cp.maxbits, cp.maxprec, cp.minexp};
    int64_t st = 1;
    for (int a = 0; a < dims; a++)
      j.n[a] = 4, j.f[a] = 0, j.e[a] = 4, j.s[a] = st, st *= 4;
    // room for the block, its padding and the decoder's look-ahead
    w.assign((std::max<uint64_t>(cp.maxbits, 16658) + std::max<uint64_t>(cp.minbits, 64)) / 64 + 8, 0);
    end = oz_compress(&j, blk.data(), w.data(), 0);
    dec.assign(blk.size(), (S)0);
    dend = oz_decompress(&j, dec.data(), w.data(), 0);
  }
};

// The words decode3 stages for one block: W = what a block can code, in words,
// plus the look-ahead word, in a slot of W | 1 words.  One more word follows:
// the next lane's slot.  WordReader::peek_at loads three dwords whatever the
// shift, so a window at the very end of a slot of W words (W odd) loads the
// first dword of the neighbour and, the shift being 0, drops it; the word is
// filled with a pattern that no stream holds, so a use of it would show.
constexpr uint64_t kNeighbour = 0xa5a5a5a5a5a5a5a5ull;
template <typename S>
static std::vector<uint64_t> staged(const Oracle& o, const CodecParams& cp, int dims)
{
  const uint32_t W = (bound_bits<S>(cp, dims) + 63) / 64 + 1;
  std::vector<uint64_t> s((W | 1u) + 1, 0);
  for (size_t i = 0; i + 1 < s.size() && i < o.w.size(); i++)
    s[i] = o.w[i];
  s.back() = kNeighbour;
  return s;
}

struct Tally {
  long blocks = 0, bad = 0;
  void fail(const char* what, int type, int dims, const CodecParams& cp, size_t blk, uint64_t got, uint64_t want)
  {
    if (bad++ < 12)
      printf("BAD %s: type %d dims %d (%u,%u,%u,%d) block %zu: %llu vs %llu\n", what, type, dims, cp.minbits,
             cp.maxbits, cp.maxprec, cp.minexp, blk, (unsigned long long)got, (unsigned long long)want);
  }
};

template <typename S>
static void run3(int type, const CodecParams& cp, const Blocks<S>& blocks, Tally& t)
{
  static const Tables tab;
  const bool rev = cp.minexp < kMinExp;
  const uint32_t bound = bound_bits<S>(cp, 3);
  // the aligned kernels' LDS: coder tables (dbl[256], lead[256]) and a slot of
  // sdw dwords, addressed by LDS byte offset; the slot ends the arena
  const uint32_t sdw = slot_dwords_for(cp.maxbits) | 1u;
  Oracle o;
  std::vector<S> od;
  for (size_t k = 0; k < blocks.size(); k++) {
    const std::vector<S>& blk = blocks[k];
    o.run(type, 3, cp, blk, od);
    auto reload = [&](S (&r)[64]) { for (int i = 0; i < 64; i++) r[i] = blk[i]; };
    S v[64];
    reload(v);
    Slot s(bound);
    OrSlot os = s.os();
    const uint32_t len = rev ? encode_block3<S, true>(os, tab.dbl.data(), v, cp, reload)
                             : encode_block3<S, false>(os, tab.dbl.data(), v, cp, reload);
    t.blocks++;
    // (padding past the slot is zeros the packer supplies: compare what the slot holds)
    if (len != o.end || !same_bits(s.base(), o.w.data(), std::min<uint64_t>(len, 64ull * s.swp)) || !s.neighbour_clean())
      t.fail("encode_block3", type, 3, cp, k, len, o.end);
    if (!rev && fixed_rate_coder_applies<S>(cp) && cp.maxbits % 64 == 0) {
      std::vector<uint32_t> arena(512 + sdw + 1, 0);
      zfp_emu_lds_base = reinterpret_cast<char*>(arena.data());
      for (int b = 0; b < 256; b++)
        arena[b] = kCoderTables.dbl[b], arena[256 + b] = kCoderTables.lead[b];
      // 8-byte aligned slot start (512 dwords in; the vector's storage is 16-byte aligned)
      OrSlot fs{reinterpret_cast<uint64_t*>(arena.data() + 512), sdw - 1};
      reload(v);
      const uint32_t flen = encode_block3<S, false, true>(fs, arena.data(), v, cp, reload);
      if (flen != o.end || !same_bits(fs.w, o.w.data(), flen))
        t.fail("encode_block3 fixed-rate coder", type, 3, cp, k, flen, o.end);
      zfp_emu_lds_base = nullptr;
    }
    const std::vector<uint64_t> st = staged<S>(o, cp, 3);
    if (sizeof(S) == 8 && !rev && cp.maxprec <= kHiPlanesMaxPrec) {
      reload(v);
      Slot hs(bound);
      OrSlot hos = hs.os();
      const uint32_t hlen = encode_block3<S, false, false, true>(hos, tab.dbl.data(), v, cp, reload);
      if (hlen != o.end || !same_bits(hs.base(), o.w.data(), std::min<uint64_t>(hlen, 64ull * hs.swp)))
        t.fail("encode_block3 planes 32..63", type, 3, cp, k, hlen, o.end);
      S dh[64];
      WordReader rh{st.data(), 0};
      const uint32_t used = decode_block3<S, false, true>(rh, tab.sq.data(), dh, cp);
      if (used != o.dend || std::memcmp(dh, od.data(), sizeof dh) != 0)
        t.fail("decode_block3 planes 32..63", type, 3, cp, k, used, o.dend);
    }
    S d[64];
    WordReader r{st.data(), 0};
    const uint32_t used = rev ? decode_block3<S, true>(r, tab.sq.data(), d, cp) : decode_block3<S, false>(r, tab.sq.data(), d, cp);
    if (used != o.dend || std::memcmp(d, od.data(), sizeof d) != 0)
      t.fail("decode_block3", type, 3, cp, k, used, o.dend);
  }
}

template <typename S, int D>
static void run_n(int type, const CodecParams& cp, const Blocks<S>& blocks, Tally& t)
{
  static const Tables tab;
  constexpr int N = 1 << (2 * D);
  const bool rev = cp.minexp < kMinExp;
  const uint32_t bound = bound_bits<S>(cp, D);
  Oracle o;
  std::vector<S> od;
  for (size_t k = 0; k < blocks.size(); k++) {
    const std::vector<S>& blk = blocks[k];
    o.run(type, D, cp, blk, od);
    S v[64] = {};
    for (int i = 0; i < N; i++)
      v[i] = blk[i];
    Slot s(bound);
    OrSlot os = s.os();
    const uint32_t len = rev ? encode_block_n<S, D, true>(os, tab.dbl.data(), v, cp)
                             : encode_block_n<S, D, false>(os, tab.dbl.data(), v, cp);
    t.blocks++;
    if (len != o.end || !same_bits(s.base(), o.w.data(), std::min<uint64_t>(len, 64ull * s.swp)) || !s.neighbour_clean())
      t.fail("encode_block_n", type, D, cp, k, len, o.end);
    const std::vector<uint64_t> st = staged<S>(o, cp, D);
    S d[64] = {};
    WordReader r{st.data(), 0};
    const uint32_t used = rev ? decode_block_n<S, D, true>(r, tab.sq.data(), d, cp)
                              : decode_block_n<S, D, false>(r, tab.sq.data(), d, cp);
    if (used != o.dend || std::memcmp(d, od.data(), N * sizeof(S)) != 0)
      t.fail("decode_block_n", type, D, cp, k, used, o.dend);
  }
}

template <typename F>
static void quad(F&& f)
{
  std::thread th[4];
  for (uint32_t r = 0; r < 4; r++)
    th[r] = std::thread([&f, r] { f(r); });
  for (auto& t : th)
    t.join();
}

// The four lane threads run through all blocks of the case (one thread start
// per case, not per block); each block has its own slot region and exchange area.
template <typename S>
static void run4(int type, const CodecParams& cp, const Blocks<S>& blocks, Tally& t)
{
  using Int = typename Traits<S>::Int;
  const bool rev = cp.minexp < kMinExp;
  uint32_t lut[256];
  for (int b = 0; b < 256; b++)
    lut[b] = dbl_entry(b);
  const uint32_t* tab = kOrderTab4.t;
  // slot / exchange region: the 4D launcher's full slot and more than 260 Ints
  const uint32_t words = std::max<uint32_t>(slot_words4(bound_bits<S>(cp, 4)), 280);
  const size_t nb = blocks.size();
  std::vector<Oracle> os(nb);
  std::vector<std::vector<S>> od(nb), dec(nb, std::vector<S>(256));
  std::vector<std::vector<uint64_t>> region(nb), xarea(nb), stg(nb);
  std::vector<uint32_t> len(4 * nb);
  for (size_t k = 0; k < nb; k++) {
    os[k].run(type, 4, cp, blocks[k], od[k]);
    region[k].assign(words + 1, 0);
    xarea[k].assign(words + 1, 0);
    // decode4 stages W = block length in words + 1 (and the exchange area aliases the staged words)
    const uint32_t W = (std::max(bound_bits<S>(cp, 4), 1u) + 63) / 64 + 1;
    stg[k].assign(std::max<uint32_t>(W | 1u, 280), 0);
    for (size_t i = 0; i < stg[k].size() && i < os[k].w.size(); i++)
      stg[k][i] = os[k].w[i];
  }
  quad([&](uint32_t r) {
    threadIdx.x = r;
    for (size_t k = 0; k < nb; k++) {
      const std::vector<S>& blk = blocks[k];
      S v[64];
      for (int i = 0; i < 64; i++)
        v[i] = blk[64 * r + i];
      auto reload = [&](S (&rr)[64]) {
        for (int i = 0; i < 64; i++)
          rr[i] = blk[64 * r + i];
      };
      uint32_t* d = reinterpret_cast<uint32_t*>(region[k].data());
      Int* X = reinterpret_cast<Int*>(xarea[k].data());
      auto place = [&](bool, uint32_t*& dd, uint32_t& jm) {
        dd = d;
        jm = 2 * words - 1;
      };
      len[4 * k + r] = rev ? encode_block4<S, true>(place, lut, tab, X, region[k].data(), words, v, cp, reload)
                           : encode_block4<S, false>(place, lut, tab, X, region[k].data(), words, v, cp, reload);
      g_bar.wait();
    }
    for (size_t k = 0; k < nb; k++) {
      WordReader rd{stg[k].data(), 0};
      S v[64];
      Int* X = reinterpret_cast<Int*>(stg[k].data());
      if (rev)
        decode_block4<S, true>(rd, v, cp, X, tab, true);
      else
        decode_block4<S, false>(rd, v, cp, X, tab, true);
      for (int i = 0; i < 64; i++)
        dec[k][64 * r + i] = v[i];
      g_bar.wait();
    }
  });
  for (size_t k = 0; k < nb; k++) {
    t.blocks++;
    const uint32_t l = len[4 * k];
    if (l != os[k].end || len[4 * k + 1] != l || len[4 * k + 2] != l || len[4 * k + 3] != l ||
        !same_bits(region[k].data(), os[k].w.data(), std::min<uint64_t>(l, 64ull * words)))
      t.fail("encode_block4", type, 4, cp, k, l, os[k].end);
    if (std::memcmp(dec[k].data(), od[k].data(), 256 * sizeof(S)) != 0)
      t.fail("decode_block4", type, 4, cp, k, 0, 0);
  }
}

template <typename S>
static void run_case(int type, int dims, const CodecParams& cp, const std::vector<int>& exps, Tally& t)
{
  static std::map<int, Blocks<S>> cache;
  if (!cache.count(dims))
    cache[dims] = make_blocks<S>(exps, 1 << (2 * dims), 77 + dims);
  const Blocks<S>& b = cache[dims];
  for (int all : {0, 1}) {  // 1: every wave-level branch entered
    emu_any_all = all;
    if (dims == 1)
      run_n<S, 1>(type, cp, b, t);
    else if (dims == 2)
      run_n<S, 2>(type, cp, b, t);
    else if (dims == 3)
      run3<S>(type, cp, b, t);
    else
      run4<S>(type, cp, b, t);
  }
  emu_any_all = false;
}

int main(int argc, char** argv)
{
  std::ifstream file;
  if (argc > 1)
    file.open(argv[1]);
  std::istream& in = argc > 1 ? static_cast<std::istream&>(file) : std::cin;
  std::map<int, std::vector<int>> exps;
  Tally t;
  long cases = 0;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string tag;
    int type;
    if (!(ls >> tag >> type) || (type != 3 && type != 4)) {
      if (!line.empty()) {
        printf("unreadable line: %s\n", line.c_str());
        return 2;
      }
      continue;
    }
    if (tag == "e") {
      int e;
      while (ls >> e)
        exps[type].push_back(e);
    } else if (tag == "p") {
      int dims;
      long long mn, mx, mp, me;
      if (!(ls >> dims >> mn >> mx >> mp >> me) || dims < 1 || dims > 4 || exps[type].empty()) {
        printf("unreadable line: %s\n", line.c_str());
        return 2;
      }
      const CodecParams cp{(uint32_t)mn, (uint32_t)mx, (uint32_t)mp, (int32_t)me};
      if (type == 3)
        run_case<float>(type, dims, cp, exps[type], t);
      else
        run_case<double>(type, dims, cp, exps[type], t);
      cases++;
    }
  }
  printf("cases %ld blocks %ld bad %ld\n", cases, t.blocks, t.bad);
  return t.bad != 0;
}
