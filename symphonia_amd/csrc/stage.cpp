// Host-pointer entry points: pinned, chunked, double-buffered staging.
//
// The device entry points assume the batch is resident in HBM.  A decoder adapter (AudioDecoder::decode gets a packet
// in host memory and must hand back a buffer in host memory) pays PCIe both ways: for a config-2 AAC batch that is 1 GiB
// each way against a quarter of a millisecond of kernel time.  The `*_pipelined` entry points -- which the plain
// host-pointer entry points of ctx.cpp route to for large batches -- cut the batch into chunks along the frame axis and
// keep three queues busy at once:
//
//      copy-in stream :  H2D(k+1) ..........
//      compute stream :  kernel(k) ......        (state carried chunk to chunk in two ping-pong device buffers)
//      copy-out stream:  D2H(k-1) ..........
//
// with two device buffer sets, so the wall time tends to max(H2D, D2H, kernel) instead of their sum.  The overlap needs
// page-locked host memory: allocate the batch buffers with symaccel_host_alloc() or pin existing ones with
// symaccel_host_register(); pageable memory still works (the runtime stages it) but serialises.
//
// Every entry point runs the same loop, run_chunks(): it alone records and waits on events, and its order (stated at its head) is
// the whole correctness argument.  An entry point checks its arguments, picks its chunk (pick_chunk), requests its buffers
// (Pipe::alloc2, State) and says what one chunk copies in, launches and copies out.
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "symaccel_internal.h"

using namespace symaccel;

namespace {

struct Pipe {
    symaccel_ctx *ctx;
    DeviceGuard dev;  // the call runs on the context's device; the caller's current device is put back behind ~Pipe's waits
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    std::vector<std::pair<void **, size_t>> wanted;
    bool queued = false;
    explicit Pipe(symaccel_ctx *c) : ctx(c), dev(c) {}
    // An early (error) return must not leave copies to or from the caller's host buffers in flight: whatever was queued is
    // waited for before the call returns.  The streams, events and the arena belong to the context and stay.
    ~Pipe() {
        if (!queued) return;
        if (s_in) (void)hipStreamSynchronize(s_in);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        if (s_out) (void)hipStreamSynchronize(s_out);
    }
    int init() {
        if (!dev.ok()) return dev.status();
        if (!ctx->stage_in) SYM_GPU(ctx, hipStreamCreate(&ctx->stage_in));
        if (!ctx->stage_out) SYM_GPU(ctx, hipStreamCreate(&ctx->stage_out));
        for (hipEvent_t &e : ctx->stage_events)
            if (!e) SYM_GPU(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        s_in = ctx->stage_in;
        s_out = ctx->stage_out;
        for (int b = 0; b < 2; ++b) {
            ev_in[b] = ctx->stage_events[b];
            ev_k[b] = ctx->stage_events[2 + b];
            ev_out[b] = ctx->stage_events[4 + b];
        }
        return SYMACCEL_OK;
    }
    // chunk buffers: requested one by one (alloc2: both halves of a double buffer), carved from the context's arena by commit()
    // (which grows it if needed; the previous call drained everything, so a smaller arena can be freed at once)
    template <class T>
    void alloc(T **p, size_t bytes) {
        *p = nullptr;
        wanted.emplace_back((void **)p, bytes);
    }
    template <class T>
    void alloc2(T *(&p)[2], size_t bytes) {
        alloc(&p[0], bytes);
        alloc(&p[1], bytes);
    }
    int commit() {
        size_t total = 0;
        for (auto &w : wanted) total += (w.second + 255) & ~(size_t)255;
        if (total > ctx->stage_arena_bytes) {
            if (ctx->stage_arena) {
                SYM_GPU(ctx, hipFree(ctx->stage_arena));
                ctx->stage_arena = nullptr;
                ctx->stage_arena_bytes = 0;
            }
            void *a = nullptr;
            SYM_TRY(ctx_alloc(ctx, &a, total, false));
            ctx->stage_arena = a;
            ctx->stage_arena_bytes = total;
        }
        size_t off = 0;
        for (auto &w : wanted) {
            *w.first = static_cast<char *>(ctx->stage_arena) + off;
            off += (w.second + 255) & ~(size_t)255;
        }
        queued = true;  // from here on work may be in flight
        return SYMACCEL_OK;
    }
    // everything queued so far, on all three streams
    // run_chunks() returns drained; a caller that goes on to queue more work says so first
    void rearm() { queued = true; }
    int drain() {
        SYM_GPU(ctx, hipStreamSynchronize(s_in));
        SYM_GPU(ctx, hipStreamSynchronize(ctx->stream));
        SYM_GPU(ctx, hipStreamSynchronize(s_out));
        queued = false;
        return SYMACCEL_OK;
    }
};

// State a chain carries from chunk to chunk, and through the caller's planes from call to call: two device copies ("sides") of the
// planes back to back.  Chunk k reads side k & 1 and writes the other one.
struct State {
    struct Plane { void *host; size_t bytes; };
    std::vector<Plane> planes;
    char *side[2];
    State(Pipe &pp, std::initializer_list<Plane> p) : planes(p) {
        size_t total = 0;
        for (const Plane &q : planes) total += q.bytes;
        pp.alloc2(side, total);
    }
    void *in(size_t k) const { return side[k & 1]; }
    void *out(size_t k) const { return side[(k + 1) & 1]; }
    // the caller's planes to (up) or from side k & 1, on the compute stream: in order with the kernels
    int copy(symaccel_ctx *ctx, size_t k, bool up) const {
        char *d = side[k & 1];
        for (const Plane &q : planes) {
            SYM_GPU(ctx, hipMemcpyAsync(up ? d : q.host, up ? q.host : d, q.bytes, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream));
            d += q.bytes;
        }
        return SYMACCEL_OK;
    }
};

// One pass over n_units units in chunks of `chunk`, chunk k in buffer set b = k & 1:
//      load(b, first, count)   queues the chunk's copies in on pp.s_in
//      compute(k, b, count)    launches its kernels on ctx->stream
//      store(b, first, count)  queues its copies out on pp.s_out
// Every chunk: ev_in[b] after the last copy in, and the compute stream waits for it; ev_k[b] after the last launch, and s_out
// waits for it; ev_out[b] after the last copy out.  Buffer set b is reused by chunk k >= 2 once chunk k-2 is through with it,
// which is waited for before anything of chunk k is queued: with separate input and output buffers, s_in waits for ev_k[b] (the
// kernels have read the input) and the compute stream for ev_out[b] (the output has left); in place, where one buffer is both,
// s_in waits for ev_out[b] alone.  `st` (may be null) is uploaded to side 0 in front of the first chunk and downloaded from the
// side the last chunk wrote.  Returns drained; a failure returns at once, and ~Pipe waits for what was queued.
template <class Load, class Compute, class Store>
int run_chunks(Pipe &pp, size_t n_units, size_t chunk, bool in_place, const State *st, Load load, Compute compute, Store store) {
    symaccel_ctx *ctx = pp.ctx;
    if (st) SYM_TRY(st->copy(ctx, 0, true));
    size_t k = 0;
    for (size_t first = 0; first < n_units; first += chunk, ++k) {
        const size_t count = std::min(chunk, n_units - first);
        const int b = (int)(k & 1);
        if (k >= 2 && in_place) {
            SYM_GPU(ctx, hipStreamWaitEvent(pp.s_in, pp.ev_out[b], 0));
        } else if (k >= 2) {
            SYM_GPU(ctx, hipStreamWaitEvent(pp.s_in, pp.ev_k[b], 0));
            SYM_GPU(ctx, hipStreamWaitEvent(ctx->stream, pp.ev_out[b], 0));
        }
        SYM_TRY(load(b, first, count));
        SYM_GPU(ctx, hipEventRecord(pp.ev_in[b], pp.s_in));
        SYM_GPU(ctx, hipStreamWaitEvent(ctx->stream, pp.ev_in[b], 0));
        SYM_TRY(compute(k, b, count));
        SYM_GPU(ctx, hipEventRecord(pp.ev_k[b], ctx->stream));
        SYM_GPU(ctx, hipStreamWaitEvent(pp.s_out, pp.ev_k[b], 0));
        SYM_TRY(store(b, first, count));
        SYM_GPU(ctx, hipEventRecord(pp.ev_out[b], pp.s_out));
    }
    if (st) SYM_TRY(st->copy(ctx, k, false));
    return pp.drain();
}

// rows x width bytes between a [rows][src_pitch] and a [rows][dst_pitch] layout
int copy_rows(symaccel_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind,
              hipStream_t s) {
    if (width == 0 || rows == 0) return SYMACCEL_OK;
    if (dpitch == width && spitch == width) {
        SYM_GPU(ctx, hipMemcpyAsync(dst, src, width * rows, kind, s));
    } else {
        SYM_GPU(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, s));
    }
    return SYMACCEL_OK;
}

constexpr size_t kChunkBytes = (size_t)32 << 20;

size_t pick_chunk(size_t units_per_chain, size_t bytes_per_unit_all_chains, size_t requested, size_t min_units) {
    if (requested > 0) return std::min(requested, units_per_chain);
    // ~32 MiB of input per chunk: large enough to fill the GPU (hundreds of wavefront segments) and to amortise the
    // per-copy latency, small enough that the first kernel starts early and the last copy-out finishes soon after the last kernel
    size_t c = kChunkBytes / std::max<size_t>(1, bytes_per_unit_all_chains);
    c = std::max(c, min_units);
    return std::min(c, units_per_chain);
}

// pair_chains (2 * n_pairs chain indices, in host memory) must name every chain at most once, inside the batch;
// pair_of[chain] = its pair, -1 for a chain no pair names
int pair_table(const int32_t *h_pair_chains, size_t n_pairs, size_t n_chains, std::vector<int32_t> *pair_of) {
    pair_of->assign(n_chains, -1);
    for (size_t p = 0; p < 2 * n_pairs; ++p) {
        const int32_t c = h_pair_chains[p];
        if (c < 0 || (size_t)c >= n_chains || (*pair_of)[(size_t)c] >= 0) return SYMACCEL_ERR_INVALID_ARG;
        (*pair_of)[(size_t)c] = (int32_t)(p / 2);
    }
    return SYMACCEL_OK;
}

}  // namespace

extern "C" {

int symaccel_host_alloc(size_t bytes, void **out) {
    if (!out) return SYMACCEL_ERR_INVALID_ARG;
    *out = nullptr;
    if (bytes == 0) bytes = 16;
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? SYMACCEL_ERR_OOM : SYMACCEL_ERR_DEVICE;
    return SYMACCEL_OK;
}

int symaccel_host_free(void *p) {
    if (!p) return SYMACCEL_OK;
    return hipHostFree(p) == hipSuccess ? SYMACCEL_OK : SYMACCEL_ERR_DEVICE;
}

int symaccel_host_register(void *p, size_t bytes) {
    if (!p || bytes == 0) return SYMACCEL_ERR_INVALID_ARG;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? SYMACCEL_OK : SYMACCEL_ERR_DEVICE;
}

int symaccel_host_unregister(void *p) {
    if (!p) return SYMACCEL_ERR_INVALID_ARG;
    return hipHostUnregister(p) == hipSuccess ? SYMACCEL_OK : SYMACCEL_ERR_DEVICE;
}

int symaccel_aac_synth_pipelined(symaccel_ctx *ctx, const float *h_coeffs, const uint8_t *h_side, float *h_delay_io, float *h_pcm,
                                 size_t n_chains, size_t frames_per_chain, size_t chunk_frames) {
    if (!ctx) return SYMACCEL_ERR_INVALID_ARG;
    if (n_chains == 0 || frames_per_chain == 0) return SYMACCEL_OK;
    if (!h_coeffs || !h_side || !h_delay_io || !h_pcm) return SYMACCEL_ERR_INVALID_ARG;
    const size_t cf = pick_chunk(frames_per_chain, n_chains * 4096, chunk_frames, 8);
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    float *d_in[2], *d_out[2];
    uint8_t *d_side[2];
    pp.alloc2(d_in, n_chains * cf * 4096);
    pp.alloc2(d_out, n_chains * cf * 4096);
    pp.alloc2(d_side, n_chains * cf);
    const State delay(pp, {{h_delay_io, n_chains * 4096}});
    SYM_TRY(pp.commit());
    return run_chunks(pp, frames_per_chain, cf, false, &delay,
        [&](int b, size_t t0, size_t nf) {
            SYM_TRY(copy_rows(ctx, d_in[b], nf * 4096, h_coeffs + t0 * 1024, frames_per_chain * 4096, nf * 4096, n_chains, hipMemcpyHostToDevice,
                              pp.s_in));
            return copy_rows(ctx, d_side[b], nf, h_side + t0, frames_per_chain, nf, n_chains, hipMemcpyHostToDevice, pp.s_in);
        },
        [&](size_t k, int b, size_t nf) {
            return launch_aac(ctx, d_in[b], d_side[b], (const float *)delay.in(k), (float *)delay.out(k), d_out[b], n_chains, nf);
        },
        [&](int b, size_t t0, size_t nf) {
            return copy_rows(ctx, h_pcm + t0 * 1024, frames_per_chain * 4096, d_out[b], nf * 4096, nf * 4096, n_chains, hipMemcpyDeviceToHost,
                             pp.s_out);
        });
}

int symaccel_aac_decode_pipelined(symaccel_ctx *ctx, const float *h_coeffs, const uint8_t *h_side, const int32_t *h_pair_chains,
                                  const symaccel_aac_js_frame *h_js_desc, size_t n_pairs, const uint16_t *swb_long, int n_swb_long,
                                  const uint16_t *swb_short, int n_swb_short, const symaccel_aac_tns_filter *h_tns, size_t n_tns,
                                  float *h_delay_io, float *h_pcm, size_t n_chains, size_t frames_per_chain, size_t chunk_frames) {
    if (!ctx) return SYMACCEL_ERR_INVALID_ARG;
    AacBandMaps maps;
    if (!aac_band_maps(swb_long, n_swb_long, swb_short, n_swb_short, &maps)) return SYMACCEL_ERR_INVALID_ARG;
    if (n_chains == 0 || frames_per_chain == 0) return SYMACCEL_OK;
    if (!h_coeffs || !h_side || !h_delay_io || !h_pcm) return SYMACCEL_ERR_INVALID_ARG;
    if ((n_pairs && (!h_pair_chains || !h_js_desc)) || (n_tns && !h_tns) || 2 * n_pairs > n_chains) return SYMACCEL_ERR_INVALID_ARG;
    if (n_chains * frames_per_chain > 0xffffffffu) return SYMACCEL_ERR_INVALID_ARG;
    std::vector<int32_t> pair_of;
    SYM_TRY(pair_table(h_pair_chains, n_pairs, n_chains, &pair_of));
    const size_t cf = pick_chunk(frames_per_chain, n_chains * 4096, chunk_frames, 8);
    const size_t n_chunks = (frames_per_chain + cf - 1) / cf;
    // TNS runs between joint stereo and the transform (ics/mod.rs:452-468), and it is a serial recurrence along the spectrum: it
    // stays a pass of its own (one lane per filter, csrc/aac_tools.hip).  The filters are sorted into the chunks of the pipeline
    // (frame indices re-based to the chunk's [chain][frame] layout); a channel-pair frame with a filter in either channel has its
    // joint stereo decoded in place IN FRONT of the filters (a list pass over those frames only) and is marked "nothing coded"
    // for the fused pair walk.  Frames without TNS -- the bulk of a stream -- are read once, by the walk.
    std::vector<std::vector<symaccel_aac_tns_filter>> tns(n_chunks);
    std::vector<std::vector<uint32_t>> tns_pf(n_chunks);
    for (size_t i = 0; i < n_tns; ++i) {
        symaccel_aac_tns_filter f = h_tns[i];
        if ((size_t)f.frame >= n_chains * frames_per_chain) continue;  // (what symaccel_aac_tns_device skips)
        const size_t chain = f.frame / frames_per_chain, t = f.frame % frames_per_chain, k = t / cf;
        const size_t nf = std::min(cf, frames_per_chain - k * cf);
        f.frame = (uint32_t)(chain * nf + (t - k * cf));
        tns[k].push_back(f);
        if (pair_of[chain] >= 0) tns_pf[k].push_back((uint32_t)((size_t)pair_of[chain] * nf + (t - k * cf)));
    }
    size_t max_tns = 0, max_pf = 0;
    for (size_t k = 0; k < n_chunks; ++k) {
        std::sort(tns_pf[k].begin(), tns_pf[k].end());
        tns_pf[k].erase(std::unique(tns_pf[k].begin(), tns_pf[k].end()), tns_pf[k].end());
        max_tns = std::max(max_tns, tns[k].size());
        max_pf = std::max(max_pf, tns_pf[k].size());
    }
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    float *d_in[2], *d_out[2];
    uint8_t *d_side[2];
    symaccel_aac_js_frame *d_js[2];
    symaccel_aac_tns_filter *d_tns[2];
    uint32_t *d_pf[2];
    int32_t *d_pairs;
    void *d_index;
    pp.alloc2(d_in, n_chains * cf * 4096);
    pp.alloc2(d_out, n_chains * cf * 4096);
    pp.alloc2(d_side, n_chains * cf);
    pp.alloc2(d_js, std::max<size_t>(1, n_pairs * cf) * sizeof(symaccel_aac_js_frame));
    pp.alloc2(d_tns, std::max<size_t>(1, max_tns) * sizeof(symaccel_aac_tns_filter));
    pp.alloc2(d_pf, std::max<size_t>(1, max_pf) * 4);
    pp.alloc(&d_pairs, std::max<size_t>(1, n_pairs) * 8);
    pp.alloc(&d_index, aac_js_scratch_bytes(n_chains, n_pairs, cf));
    const State delay(pp, {{h_delay_io, n_chains * 4096}});
    SYM_TRY(pp.commit());
    if (n_pairs) SYM_GPU(ctx, hipMemcpyAsync(d_pairs, h_pair_chains, n_pairs * 8, hipMemcpyHostToDevice, ctx->stream));
    return run_chunks(pp, frames_per_chain, cf, false, &delay,
        [&](int b, size_t t0, size_t nf) -> int {
            const size_t k = t0 / cf;
            SYM_TRY(copy_rows(ctx, d_in[b], nf * 4096, h_coeffs + t0 * 1024, frames_per_chain * 4096, nf * 4096, n_chains, hipMemcpyHostToDevice,
                              pp.s_in));
            SYM_TRY(copy_rows(ctx, d_side[b], nf, h_side + t0, frames_per_chain, nf, n_chains, hipMemcpyHostToDevice, pp.s_in));
            if (n_pairs)
                SYM_TRY(copy_rows(ctx, d_js[b], nf * sizeof(symaccel_aac_js_frame), h_js_desc + t0, frames_per_chain * sizeof(symaccel_aac_js_frame),
                                  nf * sizeof(symaccel_aac_js_frame), n_pairs, hipMemcpyHostToDevice, pp.s_in));
            if (!tns[k].empty())
                SYM_GPU(ctx, hipMemcpyAsync(d_tns[b], tns[k].data(), tns[k].size() * sizeof(symaccel_aac_tns_filter), hipMemcpyHostToDevice, pp.s_in));
            if (!tns_pf[k].empty())
                SYM_GPU(ctx, hipMemcpyAsync(d_pf[b], tns_pf[k].data(), tns_pf[k].size() * 4, hipMemcpyHostToDevice, pp.s_in));
            return SYMACCEL_OK;
        },
        [&](size_t k, int b, size_t nf) {
            if (!tns_pf[k].empty()) {  // cpe.rs:110-157 for the pair frames that carry TNS, in place; then they are plain frames for the walk
                SYM_TRY(launch_aac_joint_stereo(ctx, maps, d_in[b], nf, d_pairs, d_js[b], n_pairs, d_pf[b], tns_pf[k].size()));
                SYM_TRY(launch_aac_js_consume(ctx, d_js[b], d_pf[b], tns_pf[k].size(), n_pairs * nf));
            }
            if (!tns[k].empty()) SYM_TRY(launch_aac_tns(ctx, d_in[b], n_chains * nf, d_tns[b], tns[k].size()));  // tns.rs:180-195
            return launch_aac(ctx, d_in[b], d_side[b], (const float *)delay.in(k), (float *)delay.out(k), d_out[b], n_chains, nf,
                              n_pairs ? &maps : nullptr, d_pairs, d_js[b], n_pairs, d_index);
        },
        [&](int b, size_t t0, size_t nf) {
            return copy_rows(ctx, h_pcm + t0 * 1024, frames_per_chain * 4096, d_out[b], nf * 4096, nf * 4096, n_chains, hipMemcpyDeviceToHost,
                             pp.s_out);
        });
}

int symaccel_mp3_synth_pipelined(symaccel_ctx *ctx, const float *h_xr, const symaccel_mp3_side *h_side, int sample_rate_idx,
                                 float *h_overlap_io, float *h_vvec_io, int32_t *h_vfront_io, float *h_pcm, size_t n_chains,
                                 size_t granules_per_chain, size_t chunk_granules) {
    if (!ctx || sample_rate_idx < 0 || sample_rate_idx > 8) return SYMACCEL_ERR_INVALID_ARG;
    if (n_chains == 0 || granules_per_chain == 0) return SYMACCEL_OK;
    if (!h_xr || !h_side || !h_overlap_io || !h_vvec_io || !h_vfront_io || !h_pcm) return SYMACCEL_ERR_INVALID_ARG;
    size_t cg = pick_chunk(granules_per_chain, n_chains * 2304, chunk_granules, 8);
    if (cg < 2 && granules_per_chain >= 2) cg = 2;  // the kernel's two-granule halo wants segments of at least two
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    float *d_in[2], *d_out[2];
    symaccel_mp3_side *d_side[2];
    pp.alloc2(d_in, n_chains * cg * 2304);
    pp.alloc2(d_out, n_chains * cg * 2304);
    pp.alloc2(d_side, n_chains * cg * sizeof(symaccel_mp3_side));
    const State st(pp, {{h_overlap_io, n_chains * Mp3State::kOverlap}, {h_vvec_io, n_chains * Mp3State::kVvec}, {h_vfront_io, n_chains * Mp3State::kVfront}});
    SYM_TRY(pp.commit());
    return run_chunks(pp, granules_per_chain, cg, false, &st,
        [&](int b, size_t g0, size_t ng) {
            SYM_TRY(copy_rows(ctx, d_in[b], ng * 2304, h_xr + g0 * 576, granules_per_chain * 2304, ng * 2304, n_chains, hipMemcpyHostToDevice,
                              pp.s_in));
            return copy_rows(ctx, d_side[b], ng * 4, h_side + g0, granules_per_chain * 4, ng * 4, n_chains, hipMemcpyHostToDevice, pp.s_in);
        },
        [&](size_t k, int b, size_t ng) {
            const Mp3State si = Mp3State::carve(st.in(k), n_chains), so = Mp3State::carve(st.out(k), n_chains);
            return launch_mp3(ctx, d_in[b], d_side[b], sample_rate_idx, si.overlap, si.vvec, si.vfront, so.overlap, so.vvec, so.vfront, d_out[b],
                              n_chains, ng);
        },
        [&](int b, size_t g0, size_t ng) {
            return copy_rows(ctx, h_pcm + g0 * 576, granules_per_chain * 2304, d_out[b], ng * 2304, ng * 2304, n_chains, hipMemcpyDeviceToHost,
                             pp.s_out);
        });
}

int symaccel_mp3_decode_pipelined(symaccel_ctx *ctx, const int16_t *h_quant, const symaccel_mp3_requant *h_rq_desc,
                                  const int32_t *h_pair_chains, const symaccel_mp3_stereo *h_st_desc, size_t n_pairs,
                                  const symaccel_mp3_side *h_side, int sample_rate_idx, float *h_overlap_io, float *h_vvec_io,
                                  int32_t *h_vfront_io, float *h_pcm, size_t n_chains, size_t granules_per_chain, size_t chunk_granules) {
    if (!ctx || sample_rate_idx < 0 || sample_rate_idx > 8) return SYMACCEL_ERR_INVALID_ARG;
    if (n_chains == 0 || granules_per_chain == 0) return SYMACCEL_OK;
    if (!h_quant || !h_rq_desc || !h_side || !h_overlap_io || !h_vvec_io || !h_vfront_io || !h_pcm) return SYMACCEL_ERR_INVALID_ARG;
    if (n_pairs && (!h_pair_chains || !h_st_desc)) return SYMACCEL_ERR_INVALID_ARG;
    std::vector<int32_t> pair_of;
    SYM_TRY(pair_table(h_pair_chains, n_pairs, n_chains, &pair_of));
    // the fused kernel takes every stream as a unit: the pairs, then {chain, -1} for every chain no pair names (mono)
    std::vector<int32_t> units(h_pair_chains ? h_pair_chains : nullptr, h_pair_chains ? h_pair_chains + 2 * n_pairs : nullptr);
    for (size_t c = 0; c < n_chains; ++c)
        if (pair_of[c] < 0) {
            units.push_back((int32_t)c);
            units.push_back(-1);
        }
    const size_t n_units = units.size() / 2;
    size_t cg = pick_chunk(granules_per_chain, n_chains * 1152, chunk_granules, 8);
    if (cg < 2 && granules_per_chain >= 2) cg = 2;  // the synthesis kernel's two-granule halo wants segments of at least two
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    int16_t *d_q[2];
    symaccel_mp3_requant *d_rq[2];
    symaccel_mp3_stereo *d_st[2];
    symaccel_mp3_side *d_side[2];
    float *d_out[2];
    int32_t *d_pairs;
    pp.alloc2(d_q, n_chains * cg * 1152);
    pp.alloc2(d_rq, n_chains * cg * sizeof(symaccel_mp3_requant));
    pp.alloc2(d_st, n_units * cg * sizeof(symaccel_mp3_stereo));
    pp.alloc2(d_side, n_chains * cg * sizeof(symaccel_mp3_side));
    pp.alloc2(d_out, n_chains * cg * 2304);
    pp.alloc(&d_pairs, n_units * 8);
    const State st(pp, {{h_overlap_io, n_chains * Mp3State::kOverlap}, {h_vvec_io, n_chains * Mp3State::kVvec}, {h_vfront_io, n_chains * Mp3State::kVfront}});
    SYM_TRY(pp.commit());
    // (the requantised spectra exist in registers and LDS only: csrc/mp3.hip mp3_front)
    SYM_GPU(ctx, hipMemcpy(d_pairs, units.data(), n_units * 8, hipMemcpyHostToDevice));  // (`units` is a local: a blocking copy)
    // The stereo records of mono units are never INTERPRETED: the kernel masks the joint-stereo flags of a unit whose second chain is
    // -1 (`pair_live`, csrc/mp3.hip), whatever rows [n_pairs, n_units) hold.  They are zeroed all the same, so that what the kernel
    // loads there is defined memory.
    for (int b = 0; b < 2; ++b) SYM_GPU(ctx, hipMemsetAsync(d_st[b], 0, n_units * cg * sizeof(symaccel_mp3_stereo), pp.s_in));
    return run_chunks(pp, granules_per_chain, cg, false, &st,
        [&](int b, size_t g0, size_t ng) -> int {
            // what the entropy decoder produced: 2 bytes per line + 52-byte records (+ one 48-byte record per pair), a quarter of
            // the f32 spectra's bytes plus the side words
            SYM_TRY(copy_rows(ctx, d_q[b], ng * 1152, h_quant + g0 * 576, granules_per_chain * 1152, ng * 1152, n_chains, hipMemcpyHostToDevice, pp.s_in));
            SYM_TRY(copy_rows(ctx, d_rq[b], ng * sizeof(symaccel_mp3_requant), h_rq_desc + g0, granules_per_chain * sizeof(symaccel_mp3_requant),
                              ng * sizeof(symaccel_mp3_requant), n_chains, hipMemcpyHostToDevice, pp.s_in));
            if (n_pairs)
                SYM_TRY(copy_rows(ctx, d_st[b], ng * sizeof(symaccel_mp3_stereo), h_st_desc + g0, granules_per_chain * sizeof(symaccel_mp3_stereo),
                                  ng * sizeof(symaccel_mp3_stereo), n_pairs, hipMemcpyHostToDevice, pp.s_in));
            SYM_TRY(copy_rows(ctx, d_side[b], ng * 4, h_side + g0, granules_per_chain * 4, ng * 4, n_chains, hipMemcpyHostToDevice, pp.s_in));
            if (n_units > n_pairs && ng != cg)  // a short last chunk: the kernel indexes st_desc with stride ng, so the mono units' rows move
                SYM_GPU(ctx, hipMemsetAsync(d_st[b] + n_pairs * ng, 0, (n_units - n_pairs) * ng * sizeof(symaccel_mp3_stereo), pp.s_in));  // (defined, not needed: see above)
            return SYMACCEL_OK;
        },
        [&](size_t k, int b, size_t ng) {  // requantize, joint stereo and the synthesis tail (layer3/mod.rs:421-477) in one kernel
            const Mp3State si = Mp3State::carve(st.in(k), n_chains), so = Mp3State::carve(st.out(k), n_chains);
            return launch_mp3_decode(ctx, d_q[b], d_rq[b], d_pairs, d_st[b], n_units, d_side[b], sample_rate_idx, si.overlap, si.vvec, si.vfront,
                                     so.overlap, so.vvec, so.vfront, d_out[b], n_chains, ng);
        },
        [&](int b, size_t g0, size_t ng) {
            return copy_rows(ctx, h_pcm + g0 * 576, granules_per_chain * 2304, d_out[b], ng * 2304, ng * 2304, n_chains, hipMemcpyDeviceToHost, pp.s_out);
        });
}

// symaccel_pcm_convert_device between host buffers: chunks along the frame axis, like the synthesis entry points above.  A chunk's
// planes sit back to back on the device at a pitch that is a multiple of 4 samples and its groups' outputs at a multiple of 16 bytes,
// so that the kernel runs its aligned paths whatever the caller's strides are.
int symaccel_pcm_convert(symaccel_ctx *ctx, const void *h_src, int src_fmt, size_t plane_stride, size_t n_groups, size_t channels,
                         size_t n_frames, void *h_dst, int dst_fmt, size_t dst_group_bytes) {
    if (!ctx || !pcm_convert_shape_ok(src_fmt, plane_stride, n_groups, channels, n_frames, dst_fmt, dst_group_bytes)) return SYMACCEL_ERR_INVALID_ARG;
    if (n_groups == 0 || n_frames == 0) return SYMACCEL_OK;
    if (!h_src || !h_dst) return SYMACCEL_ERR_INVALID_ARG;
    const size_t n_planes = n_groups * channels, frame_bytes = channels * symaccel_sample_bytes(dst_fmt);
    const uintptr_t s0 = (uintptr_t)h_src, t0 = (uintptr_t)h_dst;
    const size_t src_bytes = ((n_planes - 1) * plane_stride + n_frames) * 4, dst_bytes = (n_groups - 1) * dst_group_bytes + n_frames * frame_bytes;
    if (s0 < t0 + dst_bytes && t0 < s0 + src_bytes) return SYMACCEL_ERR_INVALID_ARG;  // overlapping buffers (the chunks of an in-place call would cross)
    size_t cf = pick_chunk(n_frames, n_planes * 4, 0, 8);
    cf = std::min((cf + 3) & ~(size_t)3, (n_frames + 3) & ~(size_t)3);
    const size_t d_group_bytes = (cf * frame_bytes + 15) & ~(size_t)15;
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    uint8_t *d_in[2], *d_out[2];
    pp.alloc2(d_in, n_planes * cf * 4);
    pp.alloc2(d_out, n_groups * d_group_bytes);
    SYM_TRY(pp.commit());
    return run_chunks(pp, n_frames, cf, false, nullptr,
        [&](int b, size_t f0, size_t nf) {
            return copy_rows(ctx, d_in[b], cf * 4, static_cast<const uint8_t *>(h_src) + f0 * 4, plane_stride * 4, nf * 4, n_planes, hipMemcpyHostToDevice, pp.s_in);
        },
        [&](size_t, int b, size_t nf) {
            return launch_pcm_convert(ctx, ctx->stream, d_in[b], src_fmt, cf, n_groups, channels, nf, d_out[b], dst_fmt, d_group_bytes);
        },
        [&](int b, size_t f0, size_t nf) {
            return copy_rows(ctx, static_cast<uint8_t *>(h_dst) + f0 * frame_bytes, dst_group_bytes, d_out[b], d_group_bytes, nf * frame_bytes, n_groups,
                             hipMemcpyDeviceToHost, pp.s_out);
        });
}

// symaccel_adpcm_decode_device between host buffers: chunks of whole blocks.  On the device a chunk's blocks sit at a pitch that is a
// multiple of 16 bytes, so that every 16-byte unit of a block's image belongs to that block alone.
int symaccel_adpcm_decode(symaccel_ctx *ctx, const void *h_bytes, size_t block_pitch, size_t n_blocks, int codec, size_t channels,
                          size_t frames_per_block, void *h_pcm, int out_fmt, uint8_t *h_status) {
    if (!ctx) return SYMACCEL_ERR_INVALID_ARG;
    SYM_TRY(adpcm_shape_status(block_pitch, n_blocks, codec, channels, frames_per_block, out_fmt));
    if (n_blocks == 0) return SYMACCEL_OK;
    if (!h_bytes || !h_pcm) return SYMACCEL_ERR_INVALID_ARG;
    const size_t bytes = adpcm_block_bytes(codec, channels, frames_per_block), d_pitch = (bytes + 15) & ~(size_t)15;
    const size_t out_bytes = channels * frames_per_block * (out_fmt == 0 ? 4 : symaccel_sample_bytes(out_fmt));
    const uintptr_t s0 = (uintptr_t)h_bytes, t0 = (uintptr_t)h_pcm;
    if (s0 < t0 + n_blocks * out_bytes && t0 < s0 + (n_blocks - 1) * block_pitch + bytes) return SYMACCEL_ERR_INVALID_ARG;  // overlapping buffers
    const size_t cb = pick_chunk(n_blocks, d_pitch + out_bytes, 0, 8);
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    uint8_t *d_in[2], *d_out[2], *d_st[2];
    pp.alloc2(d_in, cb * d_pitch);
    pp.alloc2(d_out, cb * out_bytes);
    pp.alloc2(d_st, cb);
    SYM_TRY(pp.commit());
    return run_chunks(pp, n_blocks, cb, false, nullptr,
        [&](int b, size_t b0, size_t nb) {
            return copy_rows(ctx, d_in[b], d_pitch, static_cast<const uint8_t *>(h_bytes) + b0 * block_pitch, block_pitch, bytes, nb, hipMemcpyHostToDevice, pp.s_in);
        },
        [&](size_t, int b, size_t nb) {
            return launch_adpcm_decode(ctx, ctx->stream, d_in[b], d_pitch, nb, codec, (unsigned)channels, (unsigned)frames_per_block, d_out[b], out_fmt, d_st[b]);
        },
        [&](int b, size_t b0, size_t nb) -> int {
            SYM_GPU(ctx, hipMemcpyAsync(static_cast<uint8_t *>(h_pcm) + b0 * out_bytes, d_out[b], nb * out_bytes, hipMemcpyDeviceToHost, pp.s_out));
            if (h_status) SYM_GPU(ctx, hipMemcpyAsync(h_status + b0, d_st[b], nb, hipMemcpyDeviceToHost, pp.s_out));
            return SYMACCEL_OK;
        });
}

// symaccel_pcm_decode_device between host buffers.  Packets whose coded bytes and output fit a chunk go in chunks of whole packets, at
// a device pitch that is a multiple of 16 bytes; larger ones go one packet at a time in chunks of frame ranges, whose native planes
// come back row by row into the caller's planes.
int symaccel_pcm_decode(symaccel_ctx *ctx, const void *h_bytes, size_t packet_pitch, size_t n_packets, int codec, size_t channels,
                        uint32_t shift, size_t frames, void *h_pcm, int out_fmt) {
    if (!ctx) return SYMACCEL_ERR_INVALID_ARG;
    SYM_TRY(pcm_decode_shape_status(packet_pitch, n_packets, codec, channels, shift, frames, out_fmt));
    if (n_packets == 0 || frames == 0) return SYMACCEL_OK;
    if (!h_bytes || !h_pcm) return SYMACCEL_ERR_INVALID_ARG;
    const PcmCodec pc = pcm_codec(codec);
    const size_t sb = out_fmt == 0 ? pc.native : symaccel_sample_bytes(out_fmt);
    const size_t frame_in = channels * pc.coded, frame_out = channels * sb, bytes = frames * frame_in, out_bytes = frames * frame_out;
    const uintptr_t s0 = (uintptr_t)h_bytes, t0 = (uintptr_t)h_pcm;
    if (s0 < t0 + n_packets * out_bytes && t0 < s0 + (n_packets - 1) * packet_pitch + bytes) return SYMACCEL_ERR_INVALID_ARG;  // overlapping buffers
    const uint8_t *src = static_cast<const uint8_t *>(h_bytes);
    uint8_t *dst = static_cast<uint8_t *>(h_pcm);
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    uint8_t *d_in[2], *d_out[2];
    if (bytes + out_bytes <= kChunkBytes) {  // whole packets
        const size_t d_pitch = (bytes + 15) & ~(size_t)15, cp = pick_chunk(n_packets, d_pitch + out_bytes, 0, 1);
        pp.alloc2(d_in, cp * d_pitch);
        pp.alloc2(d_out, cp * out_bytes);
        SYM_TRY(pp.commit());
        return run_chunks(pp, n_packets, cp, false, nullptr,
            [&](int b, size_t p0, size_t np) { return copy_rows(ctx, d_in[b], d_pitch, src + p0 * packet_pitch, packet_pitch, bytes, np, hipMemcpyHostToDevice, pp.s_in); },
            [&](size_t, int b, size_t np) { return launch_pcm_decode(ctx, ctx->stream, d_in[b], d_pitch, np, codec, (unsigned)channels, shift, frames, d_out[b], out_fmt); },
            [&](int b, size_t p0, size_t np) -> int {
                SYM_GPU(ctx, hipMemcpyAsync(dst + p0 * out_bytes, d_out[b], np * out_bytes, hipMemcpyDeviceToHost, pp.s_out));
                return SYMACCEL_OK;
            });
    }
    // frame ranges of one packet
    const size_t cf = pick_chunk(frames, frame_in + frame_out, 0, 16);
    pp.alloc2(d_in, cf * frame_in);
    pp.alloc2(d_out, cf * frame_out);
    SYM_TRY(pp.commit());
    for (size_t p = 0; p < n_packets; ++p) {
        const uint8_t *ps = src + p * packet_pitch;
        uint8_t *pd = dst + p * out_bytes;
        pp.rearm();
        SYM_TRY(run_chunks(pp, frames, cf, false, nullptr,
            [&](int b, size_t f0, size_t nf) -> int {
                SYM_GPU(ctx, hipMemcpyAsync(d_in[b], ps + f0 * frame_in, nf * frame_in, hipMemcpyHostToDevice, pp.s_in));
                return SYMACCEL_OK;
            },
            [&](size_t, int b, size_t nf) { return launch_pcm_decode(ctx, ctx->stream, d_in[b], nf * frame_in, 1, codec, (unsigned)channels, shift, nf, d_out[b], out_fmt); },
            [&](int b, size_t f0, size_t nf) {
                if (out_fmt == 0) return copy_rows(ctx, pd + f0 * sb, frames * sb, d_out[b], nf * sb, nf * sb, channels, hipMemcpyDeviceToHost, pp.s_out);
                return copy_rows(ctx, pd + f0 * frame_out, nf * frame_out, d_out[b], nf * frame_out, nf * frame_out, 1, hipMemcpyDeviceToHost, pp.s_out);
            }));
    }
    return SYMACCEL_OK;
}

// symaccel_mpa12_decode_pp_device between host buffers: chunks of whole packets; the synthesis state ping-pongs on the device.
int symaccel_mpa12_decode(symaccel_ctx *ctx, int layer, const uint16_t *h_codes, const uint8_t *h_rec, float *h_vvec_io, int32_t *h_vfront_io,
                          float *h_pcm, uint8_t *h_status, size_t n_chains, size_t packets_per_chain) {
    if (!ctx) return SYMACCEL_ERR_INVALID_ARG;
    const size_t nf = (size_t)mpa12_n_frames(layer), rb = symaccel_mpa12_record_bytes(layer);
    if (nf == 0) return SYMACCEL_ERR_UNSUPPORTED;
    if (n_chains == 0 || packets_per_chain == 0) return SYMACCEL_OK;
    if (!h_codes || !h_rec || !h_vvec_io || !h_vfront_io || !h_pcm) return SYMACCEL_ERR_INVALID_ARG;
    if (n_chains > 0x3fffffffu || packets_per_chain > 0x3fffffffu) return SYMACCEL_ERR_INVALID_ARG;
    const size_t cb = 32 * nf * 2, pb = 32 * nf * 4;  // bytes of one channel-packet's codes / PCM
    const size_t cp = pick_chunk(packets_per_chain, n_chains * (cb + rb), 0, 8);
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    uint8_t *d_codes[2], *d_rec[2], *d_out[2], *d_st[2];
    pp.alloc2(d_codes, n_chains * cp * cb);
    pp.alloc2(d_rec, n_chains * cp * rb);
    pp.alloc2(d_out, n_chains * cp * pb);
    pp.alloc2(d_st, n_chains * cp);
    const State st(pp, {{h_vvec_io, n_chains * Mp3State::kVvec}, {h_vfront_io, n_chains * Mp3State::kVfront}});
    SYM_TRY(pp.commit());
    return run_chunks(pp, packets_per_chain, cp, false, &st,
        [&](int b, size_t p0, size_t np) -> int {
            SYM_TRY(copy_rows(ctx, d_codes[b], np * cb, reinterpret_cast<const uint8_t *>(h_codes) + p0 * cb, packets_per_chain * cb, np * cb, n_chains,
                              hipMemcpyHostToDevice, pp.s_in));
            return copy_rows(ctx, d_rec[b], np * rb, h_rec + p0 * rb, packets_per_chain * rb, np * rb, n_chains, hipMemcpyHostToDevice, pp.s_in);
        },
        [&](size_t k, int b, size_t np) {
            char *si = static_cast<char *>(st.in(k)), *so = static_cast<char *>(st.out(k));
            return launch_mpa12_decode(ctx, layer, (const uint16_t *)d_codes[b], d_rec[b], d_st[b], (const float *)si,
                                       (const int32_t *)(si + n_chains * Mp3State::kVvec), (float *)so, (int32_t *)(so + n_chains * Mp3State::kVvec),
                                       (float *)d_out[b], n_chains, np);
        },
        [&](int b, size_t p0, size_t np) -> int {
            SYM_TRY(copy_rows(ctx, h_pcm + p0 * 32 * nf, packets_per_chain * pb, d_out[b], np * pb, np * pb, n_chains, hipMemcpyDeviceToHost, pp.s_out));
            if (h_status) SYM_TRY(copy_rows(ctx, h_status + p0, packets_per_chain, d_st[b], np, np, n_chains, hipMemcpyDeviceToHost, pp.s_out));
            return SYMACCEL_OK;
        });
}

int symaccel_flac_restore_pipelined(symaccel_ctx *ctx, int32_t *h_buf, const symaccel_flac_desc *h_desc, const int32_t *h_coeffs,
                                    size_t n_blocks, size_t blocksize, size_t chunk_blocks) {
    if (!ctx || blocksize > 65535) return SYMACCEL_ERR_INVALID_ARG;
    if (n_blocks == 0 || blocksize == 0) return SYMACCEL_OK;
    if (!h_buf || !h_desc || !h_coeffs) return SYMACCEL_ERR_INVALID_ARG;
    const size_t cb = pick_chunk(n_blocks, blocksize * 4, chunk_blocks, 64);
    Pipe pp(ctx);
    SYM_TRY(pp.init());
    int32_t *d_buf[2], *d_co[2];
    symaccel_flac_desc *d_desc[2];
    pp.alloc2(d_buf, cb * blocksize * 4);
    pp.alloc2(d_co, cb * 32 * 4);
    pp.alloc2(d_desc, cb * sizeof(symaccel_flac_desc));
    SYM_TRY(pp.commit());
    return run_chunks(pp, n_blocks, cb, true /* the samples are restored where they were copied to */, nullptr,
        [&](int b, size_t b0, size_t nb) -> int {
            SYM_GPU(ctx, hipMemcpyAsync(d_buf[b], h_buf + b0 * blocksize, nb * blocksize * 4, hipMemcpyHostToDevice, pp.s_in));
            SYM_GPU(ctx, hipMemcpyAsync(d_co[b], h_coeffs + b0 * 32, nb * 32 * 4, hipMemcpyHostToDevice, pp.s_in));
            SYM_GPU(ctx, hipMemcpyAsync(d_desc[b], h_desc + b0, nb * sizeof(symaccel_flac_desc), hipMemcpyHostToDevice, pp.s_in));
            return SYMACCEL_OK;
        },
        [&](size_t, int b, size_t nb) { return launch_flac_restore(ctx, d_buf[b], d_desc[b], d_co[b], nb, blocksize); },
        [&](int b, size_t b0, size_t nb) -> int {
            SYM_GPU(ctx, hipMemcpyAsync(h_buf + b0 * blocksize, d_buf[b], nb * blocksize * 4, hipMemcpyDeviceToHost, pp.s_out));
            return SYMACCEL_OK;
        });
}

}  // extern "C"
