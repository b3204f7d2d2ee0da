// Host shim: copies between a host field and its device image, and the slab
// pipeline for a host-resident field and stream.
#pragma once

#include <chrono>
#include <condition_variable>
#include <numeric>
#include <thread>

#include "host_launch.h"

// Device-to-host copy of `bytes` into user memory that other threads may be
// filling at the same time (zfpy decompresses the chunks of one array from a
// thread pool, and chunk boundaries need not fall on pages).  The pageable
// copy path of the runtime may write whole pages, so only whole pages of the
// destination are copied directly; the partial pages at either end go through
// a private buffer and a CPU copy of exactly their bytes.
static int copy_to_host_exact(void* h, const void* d, size_t bytes, hipStream_t q, Ctx* c = nullptr)
{
  if (c && q == c->stream) {
    if (char* s = pin_take(c, bytes)) {  // small: pinned, then exactly its bytes
      HIP_TRY(hipMemcpyAsync(s, d, bytes, hipMemcpyDeviceToHost, q));
      HIP_TRY(hipStreamSynchronize(q));
      memcpy(h, s, bytes);
      return 1;
    }
  }
  constexpr uintptr_t kPage = 4096;
  const uintptr_t a = (uintptr_t)h, e = a + bytes;
  const uintptr_t a1 = (a + kPage - 1) & ~(kPage - 1), e1 = e & ~(kPage - 1);
  if (a1 >= e1) {  // no whole page inside
    std::vector<char> tmp(bytes);
    HIP_TRY(hipMemcpyAsync(tmp.data(), d, bytes, hipMemcpyDeviceToHost, q));
    HIP_TRY(hipStreamSynchronize(q));
    memcpy(h, tmp.data(), bytes);
    return 1;
  }
  const size_t head = a1 - a, tail = e - e1;
  HIP_TRY(hipMemcpyAsync((void*)a1, (const char*)d + head, e1 - a1, hipMemcpyDeviceToHost, q));
  if (head || tail) {
    std::vector<char> tmp(head + tail);
    if (head)
      HIP_TRY(hipMemcpyAsync(tmp.data(), d, head, hipMemcpyDeviceToHost, q));
    if (tail)
      HIP_TRY(hipMemcpyAsync(tmp.data() + head, (const char*)d + (e1 - a), tail, hipMemcpyDeviceToHost, q));
    HIP_TRY(hipStreamSynchronize(q));
    memcpy(h, tmp.data(), head);
    memcpy((void*)e1, tmp.data() + head, tail);
  }
  return 1;
}

// copy the box of elements between a host field and a device image of its
// span (device pointer d_base corresponds to host pointer h_base)
static int copy_box(Ctx* c, const Plan& p, void* h_base, void* d_base, size_t es, bool to_host,
                    hipStream_t q = nullptr)
{
  if (!q)
    q = c->stream;
  // whole span contiguous?  (full x/y extents, default strides)
  const Geometry& g = p.g;
  bool contiguous = true;
  int64_t expect = 1;
  for (int a = 0; a < p.dims; a++) {
    if (g.s[a] != expect)
      contiguous = false;
    expect *= (int64_t)g.n[a];
  }
  uint64_t e[4];
  for (int a = 0; a < 4; a++)
    e[a] = a < p.dims ? std::min<uint64_t>(g.n[a], g.f[a] + 4ull * g.nb[a]) : 1;
  bool full_lower = true;
  for (int a = 0; a < p.dims - 1; a++)
    if (g.f[a] != 0 || e[a] != g.n[a])
      full_lower = false;
  hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
  if ((contiguous && full_lower) || !to_host) {
    // one copy of the span (reading extra elements is harmless)
    size_t off = (size_t)p.span_lo * es;
    size_t bytes = (size_t)(p.span_hi - p.span_lo + 1) * es;
    if (to_host)
      return copy_to_host_exact((char*)h_base + off, (char*)d_base + off, bytes, q, c);
    if (q == c->stream)
      return h2d(c, (char*)d_base + off, (char*)h_base + off, bytes, q);
    HIP_TRY(hipMemcpyAsync((char*)d_base + off, (char*)h_base + off, bytes, kind, q));
    return 1;
  }
  if (g.s[0] != 1)
    return fail("zfp_hip: host-resident decompression of a non-slab chunk needs unit x stride");
  // element offset of the box's first row in slice (z, w)
  auto slice_off = [&](uint64_t z, uint64_t w) {
    return (int64_t)g.f[0] * g.s[0] + (int64_t)(p.dims >= 2 ? g.f[1] : 0) * (p.dims >= 2 ? g.s[1] : 0) +
           (int64_t)z * (p.dims >= 3 ? g.s[2] : 0) + (int64_t)w * (p.dims >= 4 ? g.s[3] : 0);
  };
  // to host: the box's rows, (z, w) slice by slice, into a private dense
  // buffer (2D copies), then row by row into the field (neighbouring boxes of
  // the same array may be written concurrently, and the pageable copy path may
  // write whole pages)
  if (to_host) {
    const size_t w0 = (size_t)(e[0] - g.f[0]) * es;
    const size_t nrows = p.dims >= 2 ? (size_t)(e[1] - g.f[1]) : 1;
    // a negative y stride (rows stored last to first): the 2D copy starts at
    // the slice's last row, the lowest address, and the rows go back reversed
    const int64_t sy = nrows > 1 ? g.s[1] : 0;
    const bool flip = sy < 0;
    const size_t pitch = nrows > 1 ? (size_t)(flip ? -sy : sy) * es : w0;
    if (pitch < w0)
      return fail("zfp_hip: host-resident decompression needs a y stride of at least the row length");
    const int64_t low_row = flip ? (int64_t)(nrows - 1) * sy : 0;
    const uint64_t z0 = p.dims >= 3 ? g.f[2] : 0, z1 = p.dims >= 3 ? e[2] : 1;
    const uint64_t v0 = p.dims >= 4 ? g.f[3] : 0, v1 = p.dims >= 4 ? e[3] : 1;
    std::vector<char> tmp(w0 * nrows * (size_t)((z1 - z0) * (v1 - v0)));
    size_t k = 0;
    for (uint64_t w = v0; w < v1; w++)
      for (uint64_t z = z0; z < z1; z++, k++)
        HIP_TRY(hipMemcpy2DAsync(tmp.data() + k * w0 * nrows, w0,
                                 (char*)d_base + (slice_off(z, w) + low_row) * (int64_t)es, pitch, w0, nrows,
                                 hipMemcpyDeviceToHost, q));
    HIP_TRY(hipStreamSynchronize(q));
    k = 0;
    for (uint64_t w = v0; w < v1; w++)
      for (uint64_t z = z0; z < z1; z++, k++)
        for (size_t y = 0; y < nrows; y++)
          memcpy((char*)h_base + (slice_off(z, w) + (int64_t)y * (p.dims >= 2 ? g.s[1] : 0)) * (int64_t)es,
                 tmp.data() + (k * nrows + (flip ? nrows - 1 - y : y)) * w0, w0);
    return 1;
  }
  // row-wise 2D copies, one per (z, w) slice
  size_t width = (size_t)(e[0] - g.f[0]) * es;
  size_t rows = p.dims >= 2 ? (size_t)(e[1] - g.f[1]) : 1;
  size_t pitch = (size_t)(p.dims >= 2 ? g.s[1] : 1) * es;
  for (uint64_t w = (p.dims >= 4 ? g.f[3] : 0); w < (p.dims >= 4 ? e[3] : 1); w++)
    for (uint64_t z = (p.dims >= 3 ? g.f[2] : 0); z < (p.dims >= 3 ? e[2] : 1); z++) {
      const int64_t off = slice_off(z, w);
      HIP_TRY(hipMemcpy2DAsync((char*)h_base + off * (int64_t)es, pitch, (char*)d_base + off * (int64_t)es, pitch,
                               width, rows, kind, q));
    }
  return 1;
}

// Host-resident field and stream: slab pipeline.  The chunk is
// cut along its outermost axis into slabs of whole block layers (default about
// 128 MB of field each).  Three host threads drive three HIP streams:
//   uploads    field slab s (compress) / stream words of slab s (decompress)
//   kernels    slab s once its upload is done (a device-side event wait)
//   downloads  stream words / field slab s once its kernel is done
// so the two PCIe directions run at once (pageable copies from two threads: 83
// GB/s together on the box, 57 and 55 alone) and the kernels hide under them.
// Slab s is an ordinary chunk encode at bit offset O_s: fixed rate O_s is
// analytic; variable rate O_s = O_{s-1} + its length, known when slab s-1's
// kernel returns (the look-back runs within a slab).  The word holding O_s is
// shared by two slabs: slab s keeps the bits slab s-1 left below its first bit
// (Head::keep), and slab s-1's download stops before that word.  Every slab has
// its own region of the device images, so no buffer is reused while a copy of
// it may be in flight.
static uint64_t env_mb(const char* name, uint64_t dflt)
{
  if (const char* e = getenv(name)) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v)
      return v << 20;
  }
  return dflt << 20;
}

struct Slab {
  zfp_hip_job job;
  Plan p;
  uint64_t b0;  // first block of the slab within the chunk
};

// Slabs of whole block layers along the outermost axis; false: the chunk is
// not worth (or not fit for) the pipeline.  Variable rate: slabs hold whole
// waves (the chunk's block index layout).
static bool make_slabs(const zfp_hip_job* job, const void* field_base, const Plan& p, std::vector<Slab>& out)
{
  const uint64_t align = p.fixed ? 1 : p.per_wave;
  const size_t es = p.es;
  if (p.span_bytes() < env_mb("ZFP_HIP_PIPE_MIN_MB", 256))
    return false;
  // contiguous layout: each slab's span is its own range of the field
  int64_t expect = 1;
  for (int a = 0; a < p.dims; a++) {
    if (p.g.s[a] != expect)
      return false;
    expect *= (int64_t)p.g.n[a];
  }
  const int ao = p.dims - 1;
  const uint64_t nbo = p.g.nb[ao];
  if (nbo < 2)
    return false;
  const uint64_t layer = p.g.nblocks / nbo;
  const uint64_t layer_bytes = layer * (1ull << (2 * p.dims)) * es;
  uint64_t L = std::max<uint64_t>(1, env_mb("ZFP_HIP_PIPE_SLAB_MB", 128) / layer_bytes);
  if (align > 1) {
    const uint64_t q = align / std::gcd(layer, align);
    L = (L + q - 1) / q * q;
  }
  if (L >= nbo)
    return false;
  for (uint64_t l0 = 0; l0 < nbo; l0 += L) {
    Slab sl;
    sl.job = *job;
    sl.job.f[ao] = job->f[ao] + 4 * l0;
    sl.job.e[ao] = std::min<uint64_t>(job->e[ao], job->f[ao] + 4 * (l0 + L));
    if (!plan_job(&sl.job, field_base, sl.p))
      return false;
    sl.b0 = l0 * layer;
    out.push_back(sl);
  }
  return true;
}

static int ensure_side_streams(Ctx* c)
{
  for (auto& q : c->side)
    if (!q)
      HIP_TRY(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
  return 1;
}

// Hand-off between the pipeline's host threads: `done[k]` counts the slabs
// whose stage-k event is recorded (a stream can only wait for a recorded event).
struct PipeSync {
  std::mutex mu;
  std::condition_variable cv;
  size_t done[2] = {0, 0};
  bool failed = false;
  std::string err;
  void post(int k, size_t n)
  {
    { std::lock_guard<std::mutex> l(mu); done[k] = n; }
    cv.notify_all();
  }
  void fail_with(const char* what)
  {
    { std::lock_guard<std::mutex> l(mu); if (!failed) { failed = true; err = what; } }
    cv.notify_all();
  }
  bool wait(int k, size_t n)  // false: another stage failed
  {
    std::unique_lock<std::mutex> l(mu);
    cv.wait(l, [&] { return failed || done[k] >= n; });
    return !failed;
  }
};

struct EventSet {
  std::vector<hipEvent_t> ev;
  explicit EventSet(size_t n) : ev(n, nullptr)
  {
    for (auto& e : ev)
      (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  }
  ~EventSet()
  {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// The pipeline over `ns` slabs.  The three callables say what slab s queues and
// return 0 on failure: upload(s) its input on side[0] (upload thread),
// launch(s) its kernels on c->stream (calling thread), download(s) its output
// on side[1] (download thread).  launch(s) runs once upload(s) is queued, with
// the stream waiting for it; download(s) once launch(s) has returned, so it
// may use what launch(s) worked out on the host.  Every queued copy has
// finished when this returns, failed or not.  `who` names the entry point,
// `in` and `out` what is uploaded and downloaded (error messages).
template <typename Up, typename Launch, typename Down>
static int run_slabs(Ctx* c, size_t ns, const char* who, const char* in, const char* out, Up upload, Launch launch,
                     Down download)
{
  if (!ensure_side_streams(c))
    return 0;
  EventSet ev_in(ns), ev_k(ns);
  PipeSync ps;
  const std::string up_err = std::string(in) + " upload failed", down_err = std::string(out) + " download failed";
  std::thread up([&] {
    if (hipSetDevice(c->device) != hipSuccess)
      return ps.fail_with("hipSetDevice failed (upload thread)");
    for (size_t s = 0; s < ns; s++) {
      if (!upload(s) || hipEventRecord(ev_in.ev[s], c->side[0]) != hipSuccess)
        return ps.fail_with(up_err.c_str());
      ps.post(0, s + 1);
    }
  });
  std::thread down([&] {
    if (hipSetDevice(c->device) != hipSuccess)
      return ps.fail_with("hipSetDevice failed (download thread)");
    for (size_t s = 0; s < ns; s++) {
      if (!ps.wait(1, s + 1))
        return;
      if (hipStreamWaitEvent(c->side[1], ev_k.ev[s], 0) != hipSuccess || !download(s))
        return ps.fail_with(down_err.c_str());
    }
    if (hipStreamSynchronize(c->side[1]) != hipSuccess)
      ps.fail_with(down_err.c_str());
  });
  int ok = 1;  // 0: this thread's stage failed, g_err says why
  for (size_t s = 0; s < ns && ok && ps.wait(0, s + 1); s++) {
    if (hipStreamWaitEvent(c->stream, ev_in.ev[s], 0) != hipSuccess)
      ok = fail("hipStreamWaitEvent failed");
    else if (!launch(s))
      ok = 0;
    else if (hipEventRecord(ev_k.ev[s], c->stream) != hipSuccess)
      ok = fail("hipEventRecord failed");
    else
      ps.post(1, s + 1);
  }
  if (!ok)
    ps.fail_with(g_err.c_str());
  up.join();
  down.join();
  hipError_t e = hipSuccess;
  for (hipStream_t q : {c->stream, c->side[0], c->side[1]})
    if (hipError_t eq = hipStreamSynchronize(q); eq != hipSuccess)
      e = eq;
  if (!ok)
    return 0;
  if (ps.failed)
    return fail("%s: %s", who, ps.err.c_str());
  if (e != hipSuccess)
    return fail("%s: hipStreamSynchronize failed: %s", who, hipGetErrorString(e));
  return 1;
}

// The pipelined path has no kernel time of its own to report: kernel_ms stays
// 0 and total_ms is the wall time of `call`.
template <typename F>
static int timed_wall(F&& call)
{
  const auto t0 = std::chrono::steady_clock::now();
  const int ok = call();
  t_timing.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  t_timing.kernel_ms = 0;
  t_timing.timed = ok != 0;
  return ok;
}

// Slab s is encoded at the bit where slab s-1 ended, into its own words of the
// chunk's device stream image; its download takes the words it completed.
template <typename S>
static int compress_slabs(Ctx* c, const Plan& p, const std::vector<Slab>& sl, const void* field_base,
                          uint64_t* words, uint64_t capacity_words, uint64_t bit_offset, uint64_t head_word,
                          zfp_hip_index* index, uint64_t* end_bit)
{
  const size_t ns = sl.size();
  const uint64_t W0 = bit_offset >> 6;
  const uint64_t worst_bits = (bit_offset & 63) + p.g.nblocks * (uint64_t)(p.fixed ? p.cp.maxbits : p.max_len);
  char* d_img;
  if (!field_image(c, p, &d_img) || !ensure(c->words, ((worst_bits + 63) / 64 + 1) * 8))
    return 0;
  uint64_t* d_words = (uint64_t*)c->words.p;
  if (p.fixed)
    index = nullptr;
  if (index && !index_begin(index, c, p))
    return 0;
  std::vector<uint64_t> wa(ns), wb(ns);  // stream words [wa, wb) of slab s, relative to W0
  uint64_t off = bit_offset;             // where the next slab starts
  const int ok = run_slabs(
      c, ns, "zfp_hip_compress", "field", "stream",
      [&](size_t s) { return copy_box(c, sl[s].p, (void*)field_base, d_img, sizeof(S), false, c->side[0]); },
      [&](size_t s) {
        const uint64_t Ws = off >> 6;
        const Head h{s == 0 ? head_word : 0ull, s > 0, off - bit_offset};
        IndexView view;  // the slab's part of the chunk's index
        if (index)
          view = index_view(index, sl[s].b0, sl[s].p);
        uint64_t total = 0;
        if (!launch_encode<S>(c, sl[s].p, (const S*)d_img, d_words + (Ws - W0), (uint32_t)(off & 63), h,
                              index ? &view : nullptr, &total))
          return 0;
        off += total;
        wa[s] = Ws - W0;
        wb[s] = (s + 1 < ns ? off >> 6 : (off + 63) >> 6) - W0;
        if (W0 + wb[s] > capacity_words)
          return fail("zfp_hip_compress: compressed stream (%llu words) exceeds capacity %llu",
                      (unsigned long long)(W0 + wb[s]), (unsigned long long)capacity_words);
        return 1;
      },
      [&](size_t s) {
        return hipMemcpyAsync(words + W0 + wa[s], d_words + wa[s], (wb[s] - wa[s]) * 8, hipMemcpyDeviceToHost,
                              c->side[1]) == hipSuccess;
      });
  if (!ok || (index && !index_publish(c, index, p, words, false, bit_offset, off - bit_offset)))
    return 0;
  *end_bit = off;
  return 1;
}

// Slab s's stream words are known before any kernel runs: fixed rate
// analytically, variable rate from the block index (the start of the slab's
// first wave; slabs hold whole waves), whose per-slab bases are read back
// first.  Every slab decodes against the chunk's whole stream image, with its
// view of the index, once its own words have arrived.
template <typename S>
static int decompress_slabs(Ctx* c, const Plan& p, const std::vector<Slab>& sl, void* field_base,
                            const uint64_t* words, uint64_t capacity_words, uint64_t bit_offset,
                            const zfp_hip_index* index, uint64_t* end_bit)
{
  const size_t ns = sl.size();
  const StreamPos at(bit_offset, capacity_words);
  const uint64_t W0 = at.W0, g0 = at.g0, mb = p.cp.maxbits;
  const uint64_t total = p.fixed ? p.g.nblocks * mb : index->total_bits;
  const uint64_t nwords = at.decode_words(total);
  char* d_img;
  if (!field_image(c, p, &d_img) || !ensure(c->words, nwords * 8 + 8))
    return 0;
  uint64_t* d_words = (uint64_t*)c->words.p;
  // bit offset of slab s's first block relative to the chunk's first block
  std::vector<uint64_t> base(ns + 1, total);
  for (size_t s = 0; s < ns; s++) {
    if (p.fixed)
      base[s] = sl[s].b0 * mb;
    else
      HIP_TRY(hipMemcpyAsync(&base[s], index->d_base + sl[s].b0 / p.per_wave, 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  // stream words [wa, wb) relative to W0 read by slab s (one word of lookahead)
  std::vector<uint64_t> wa(ns), wb(ns);
  for (size_t s = 0; s < ns; s++) {
    if (base[s] > base[s + 1] || base[s + 1] > total)
      return fail("zfp_hip_decompress: block index inconsistent with the slab layout");
    wa[s] = (g0 + base[s]) >> 6;
    wb[s] = std::min<uint64_t>(((g0 + base[s + 1] + 63) >> 6) + 1, nwords);
  }
  const int ok = run_slabs(
      c, ns, "zfp_hip_decompress", "stream", "field",
      [&](size_t s) {
        return hipMemcpyAsync(d_words + wa[s], words + W0 + wa[s], (wb[s] - wa[s]) * 8, hipMemcpyHostToDevice,
                              c->side[0]) == hipSuccess;
      },
      [&](size_t s) {
        if (p.fixed)
          return launch_decode<S>(c, sl[s].p, (S*)d_img, d_words + wa[s], wb[s] - wa[s],
                                  (uint32_t)((bit_offset + base[s]) & 63), nullptr);
        IndexView view = index_view(index, sl[s].b0, sl[s].p);
        view.total_bits = base[s + 1] - base[s];
        return launch_decode<S>(c, sl[s].p, (S*)d_img, d_words, nwords, at.g0, &view);
      },
      [&](size_t s) { return copy_box(c, sl[s].p, field_base, d_img, sizeof(S), true, c->side[1]); });
  if (!ok)
    return 0;
  *end_bit = bit_offset + total;
  return 1;
}
