// Internal declarations shared by the host side of libsymaccel (not part of the ABI).
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/symaccel.h"
#include <hip/hip_runtime.h>

namespace symaccel {

struct cpx {
    float re, im;
};

constexpr int kMp3Pow2abMinE = -1300, kMp3Pow2abLen = 1346;  // exponents a - b of requantize.rs:280, 343
constexpr int kMp3Unscaled = 39;                             // band-map value of lines no band covers

// Constant tables, generated on the host with the libm calls the reference uses (tables.cpp).
struct HostTables {
    // AAC (symphonia-codec-aac/src/aac/window.rs:28-63, dsp.rs:34-54)
    std::vector<float> aac_kbd_long, aac_kbd_short, aac_sine_long, aac_sine_short;
    std::vector<cpx> aac_tw_long, aac_tw_short;  // Imdct twiddles N=1024 (scale 1/2048), N=128 (1/256)
    // FFT (symphonia-core/src/dsp/fft/no_simd.rs:16-36, 307-324, 374-383)
    std::vector<cpx> fft_merge;   // W64 | W128 | ... | W4096 back to back (offset of W_n = n/2 - 32)
    cpx small16[8], small32[16];  // combine constants of fft16 / fft32 in "general form"
    uint8_t small16_form[8], small32_form[16];  // 0 general, 1 identity, 2 multiply by -i
    // MP3 (hybrid_synthesis.rs:53-149, 611-630, 668-678, 722-730; synthesis.rs:13-142, 354-396)
    float mp3_imdct_win[4][36];
    float mp3_cos12[6][6];
    float mp3_cs[8], mp3_ca[8];
    float mp3_dct_iv_scale[18], mp3_sdct18_scale[9], mp3_sdct9_d[7];
    float mp3_cos16[16], mp3_cos8[8], mp3_cos4[4], mp3_cos2[2], mp3_cos1;
    float mp3_synth_d[512];
    int32_t mp3_sfb_short[9][40];
    int32_t mp3_sfb_mixed[9][40];
    int32_t mp3_sfb_mixed_len[9];
    int32_t mp3_sfb_switch[9];
    // MP3 requantisation (requantize.rs:28-31, 256-257, 280, 343; layer3/common.rs:9-56)
    int32_t mp3_sfb_long[9][23];
    float mp3_pow43[8207];
    float mp3_pow2ab[kMp3Pow2abLen];
    uint8_t mp3_band_map[9][4][576];  // [sample rate][long, short, mixed (requantize), mixed (stereo)][line] -> band / slot
                                      // index; kMp3Unscaled = no band (requantize's mixed map only)
    float mp3_is_ratios[7 + 64][2];   // INTENSITY_STEREO_RATIOS_MPEG1[7] | _MPEG2[2][32] as (left, right) (stereo.rs:31-118)
    // Vorbis (floor.rs:21-112)
    float vorbis_floor1_db[256];
    // MPEG Layer I / II dequantisation, packed as Mpa12Layout (layer1/mod.rs:19-47, layer12.rs:9-76, layer2/mod.rs:46-64)
    float mpa12[131];
};

const HostTables &host_tables();
void make_imdct_twiddles(int n, double scale, cpx *dst);  // mdct.rs:45-54
void make_fft_twiddles(int n, cpx *dst);                  // no_simd.rs:16-36
void make_vorbis_window(int bs, float *dst);              // vorbis window.rs:11-24

inline size_t fft_merge_offset(int n) { return (size_t)(n / 2 - 32); }  // n >= 64

// Device-resident copy of the tables the kernels read (plain pointers, passed by value).
struct DevTables {
    const float *aac_kbd_long, *aac_kbd_short, *aac_sine_long, *aac_sine_short;
    const cpx *aac_tw_long, *aac_tw_short;
    const cpx *fft_merge;
    const cpx *small16, *small32;        // 8 + 16 complex
    const uint8_t *small16_form, *small32_form;
    const float *mp3_consts;             // packed, see Mp3ConstLayout
    const int32_t *mp3_reorder_map;      // [9 sample rates][2 (plain, mixed)][576] source index
    const int32_t *mp3_reorder_end;      // [9][2][577]: reorder end index `i` for each input rzero
    const float *vorbis_floor1_db;
    const float *mp3_pow43, *mp3_pow2ab;
    const uint8_t *mp3_band_map;         // [9][4][576]
    const float *mp3_is_ratios;          // [71][2]
    const float *mpa12;                  // packed, see Mpa12Layout
};

// Offsets (in floats) inside DevTables::mp3_consts.
enum Mp3ConstLayout {
    MP3C_IMDCT_WIN = 0,    // 4*36
    MP3C_COS12 = 144,      // 36
    MP3C_CS = 180,         // 8
    MP3C_CA = 188,         // 8
    MP3C_DCT_IV = 196,     // 18
    MP3C_SDCT18 = 214,     // 9
    MP3C_SDCT9_D = 223,    // 7
    MP3C_COS16 = 230,      // 16
    MP3C_COS8 = 246,       // 8
    MP3C_COS4 = 254,       // 4
    MP3C_COS2 = 258,       // 2
    MP3C_COS1 = 260,       // 1
    MP3C_SYNTH_D = 264,    // 512
    MP3C_TOTAL = 776
};

// Offsets (in floats) inside HostTables::mpa12 / DevTables::mpa12 (SYMACCEL_TABLE_MPA12).
constexpr int kMpa12Classes = 17;  // QUANT_CLASS, layer2/mod.rs:46-64
enum Mpa12Layout {
    MPA12_FACTOR = 0,   // 16: FACTOR[bits], entries 0 and 1 are 0.0 (layer1/mod.rs:19-47)
    MPA12_SCF = 16,     // 64: LAYER12_SCALEFACTORS (layer12.rs:9-76)
    MPA12_CLASS = 80,   // 17 x {c, d, sample width}: bits, or for a grouped class the bits that hold nlevels (layer2/mod.rs:183)
    MPA12_TOTAL = 131
};
// time slots per packet and channel of a layer (layer1/mod.rs:193, layer2/mod.rs:383), 0 for anything else
constexpr int mpa12_n_frames(int layer) { return layer == SYMACCEL_MPA_LAYER1 ? 12 : layer == SYMACCEL_MPA_LAYER2 ? 36 : 0; }

struct ImdctPlan {
    int n;
    cpx *d_twiddle;  // n/2 complex on the device
};

}  // namespace symaccel

struct symaccel_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    int segment = 0;  // 0 = choose per launch (choose_segment)
    int n_cus = 256;  // compute units of the device (MI355X: 256)
    std::string last_error;
    symaccel::DevTables dev{};
    std::vector<void *> allocations;  // freed on destroy
    std::map<std::pair<int, uint64_t>, symaccel::ImdctPlan> imdct_plans;
    std::map<int, float *> vorbis_windows;  // bs -> device window (bs/2 floats)
    // growable device scratch (state double-buffering, per-block offsets)
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    // host <-> device staging of the *_pipelined entry points (stage.cpp), created on first use and kept: two copy streams,
    // six events, one growable device arena the chunk buffers are carved from
    hipStream_t stage_in = nullptr, stage_out = nullptr;
    hipEvent_t stage_events[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    void *stage_arena = nullptr;
    size_t stage_arena_bytes = 0;
    // small dedicated device buffers (not shared with `scratch`, whose growth synchronises the stream)
    void *sink = nullptr;  // 2 MiB nobody reads: target of the stores of wavefronts / lanes that must not emit (ctx_sink)
    void *alac_flags = nullptr;
    size_t alac_flags_bytes = 0;
};

namespace symaccel {

int ctx_fail(symaccel_ctx *ctx, hipError_t err, const char *where);
int ctx_alloc(symaccel_ctx *ctx, void **out, size_t bytes, bool tracked = true);
int ctx_scratch(symaccel_ctx *ctx, size_t bytes, void **out);
// The context's sink buffer (kSinkBytes, allocated on first use, never read).  Kernels whose loops must issue a FIXED number of
// stores per round (the vmcnt bookkeeping of aac.hip / mp3.hip) aim the stores of halo rounds at a slot of it.
constexpr size_t kSinkBytes = 2u << 20;
int ctx_sink(symaccel_ctx *ctx, void **out);
int ctx_upload(symaccel_ctx *ctx, const void *src, size_t bytes, const void **out);
int get_imdct_plan(symaccel_ctx *ctx, int n, double scale, const ImdctPlan **out);
unsigned choose_segment(const symaccel_ctx *ctx, size_t n_chains, size_t frames_per_chain, unsigned waves_per_cu,
                        unsigned items_per_wave, unsigned halo, unsigned min_seg);
int get_vorbis_window(symaccel_ctx *ctx, int bs, const float **out);

// Entry points run on the context's device and leave the caller's current device as they found it (a process that
// drives several GPUs through one thread must not have its "current device" moved by a library call).
class DeviceGuard {
public:
    explicit DeviceGuard(symaccel_ctx *ctx) {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        if (prev_ != ctx->device) {
            const hipError_t e = hipSetDevice(ctx->device);
            if (e != hipSuccess) {
                status_ = ctx_fail(ctx, e, "hipSetDevice");
                prev_ = -1;
            } else {
                switched_ = true;
            }
        }
    }
    ~DeviceGuard() {
        if (switched_ && prev_ >= 0) (void)hipSetDevice(prev_);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    bool ok() const { return status_ == SYMACCEL_OK; }
    int status() const { return status_; }

private:
    int prev_ = -1;
    int status_ = SYMACCEL_OK;
    bool switched_ = false;
};

#define SYM_TRY(expr)                                                   \
    do {                                                                \
        int _st = (expr);                                               \
        if (_st != SYMACCEL_OK) return _st;                             \
    } while (0)
#define SYM_GPU(ctx, expr)                                              \
    do {                                                                \
        hipError_t _e = (expr);                                         \
        if (_e != hipSuccess) return ::symaccel::ctx_fail((ctx), _e, #expr); \
    } while (0)

// line / 4 -> scale-factor band of the caller's swb offset tables (255 = past the last band), passed by value
struct AacBandMaps {
    uint8_t long4[256];
    uint8_t short4[32];
};

// kernel launchers (one per .hip file)
int launch_fft_big_wave(symaccel_ctx *ctx, int n, const float *d_in, float *d_out, size_t count, bool inverse);            // imdct_big.hip
int launch_fft4096_wg(symaccel_ctx *ctx, const float *d_in, float *d_out, size_t count, bool inverse);                         // imdct_big.hip
int launch_imdct8192_wg(symaccel_ctx *ctx, const cpx *d_twiddle, const float *d_spec, float *d_out, size_t count);              // imdct_big.hip
int launch_imdct_big_wave(symaccel_ctx *ctx, const cpx *d_twiddle, int nf, const float *d_spec, float *d_out, size_t count);  // imdct_big.hip
int launch_fft(symaccel_ctx *ctx, int n, const float *d_in, float *d_out, size_t count, bool inverse = false);
int launch_imdct(symaccel_ctx *ctx, const ImdctPlan &plan, const float *d_spec, float *d_out, size_t count);
// (maps / d_pair_chains / d_js_desc / n_pairs / d_js_scratch: joint stereo on load, symaccel_aac_synth_js_*; scratch of
// aac_js_scratch_bytes(n_chains, n_pairs, frames_per_chain) bytes)
int launch_aac(symaccel_ctx *ctx, const float *d_coeffs, const uint8_t *d_side, const float *d_delay_in,
               float *d_delay_out, float *d_pcm, size_t n_chains, size_t frames_per_chain, const AacBandMaps *maps = nullptr,
               const int32_t *d_pair_chains = nullptr, const symaccel_aac_js_frame *d_js_desc = nullptr, size_t n_pairs = 0,
               void *d_js_scratch = nullptr);
inline size_t aac_js_scratch_bytes(size_t n_chains, size_t n_pairs, size_t frames_per_chain) {
    (void)n_pairs;
    (void)frames_per_chain;
    return ((n_chains * 8 + 255) & ~(size_t)255) + 256;
}
// The state an MP3 chain carries from call to call, as three planes back to back in one device block (k*: bytes per chain)
struct Mp3State {
    float *overlap;   // [n_chains][576]
    float *vvec;      // [n_chains][1024]
    int32_t *vfront;  // [n_chains]
    static constexpr size_t kOverlap = 576 * 4, kVvec = 1024 * 4, kVfront = 4;
    static size_t bytes(size_t n_chains) { return n_chains * (kOverlap + kVvec + kVfront); }
    static Mp3State carve(void *base, size_t n_chains) {
        char *p = static_cast<char *>(base);
        return {(float *)p, (float *)(p + n_chains * kOverlap), (int32_t *)(p + n_chains * (kOverlap + kVvec))};
    }
};
int launch_mp3(symaccel_ctx *ctx, const float *d_xr, const symaccel_mp3_side *d_side, int sr,
               const float *d_overlap_in, const float *d_vvec_in, const int32_t *d_vfront_in,
               float *d_overlap_out, float *d_vvec_out, int32_t *d_vfront_out, float *d_pcm,
               size_t n_chains, size_t granules_per_chain);
int launch_vorbis(symaccel_ctx *ctx, int bs0_exp, int bs1_exp, const float *d_spectra, const float *d_residue,
                  size_t spec_stride,
                  const uint8_t *d_block_flag, const int32_t *d_prev_in, int32_t *d_prev_out,
                  const float *d_overlap_in, float *d_overlap_out, float *d_pcm, size_t pcm_stride,
                  size_t n_chains, size_t blocks_per_chain, void *d_offsets, const uint8_t *d_floor_y = nullptr);
int launch_vorbis_wave(symaccel_ctx *ctx, const cpx *tw_short, const cpx *tw_long, const float *win_short,
                       const float *win_long, const float *d_spectra, const float *d_residue, size_t spec_stride,
                       const uint8_t *d_block_flag,
                       const int32_t *d_prev_in, int32_t *d_prev_out, const float *d_overlap_in, float *d_overlap_out,
                       float *d_pcm, size_t pcm_stride, size_t n_chains, unsigned nb, unsigned seg, int floor_mode);
// SYM_VORBIS_WG (build knob): 1 = pairs with long blocks of 8192 samples run the workgroup-cooperative vorbis_synth_wg_kernel, 2 = those
// with 4096-sample long blocks too, 0 = vorbis_synth_wave2_kernel's one-wavefront-per-block form for all of them (kept for the A/B).
#ifndef SYM_VORBIS_WG
#define SYM_VORBIS_WG 1
#endif
#ifndef SYM_VORBIS_WG_SHARED
#define SYM_VORBIS_WG_SHARED 1  // vorbis_wg.hip: exchange / group work areas inside the staging area, three workgroups per CU
#endif
int launch_vorbis_wg(symaccel_ctx *ctx, int bs0_exp, int bs1_exp, const cpx *tw_short, const cpx *tw_long, const float *win_short,
                     const float *win_long, const float *d_spectra, const float *d_residue, size_t spec_stride, const uint8_t *d_block_flag,
                     const int32_t *d_prev_in, int32_t *d_prev_out, const float *d_overlap_in, float *d_overlap_out, float *d_pcm,
                     size_t pcm_stride, size_t n_chains, unsigned nb, unsigned seg, int floor_mode);  // vorbis_wg.hip
int launch_vorbis_wave2(symaccel_ctx *ctx, int bs0_exp, int bs1_exp, const cpx *tw_short, const cpx *tw_long, const float *win_short,
                        const float *win_long, const float *d_spectra, const float *d_residue, size_t spec_stride,
                        const uint8_t *d_block_flag, const int32_t *d_prev_in, int32_t *d_prev_out, const float *d_overlap_in,
                        float *d_overlap_out, float *d_pcm, size_t pcm_stride, size_t n_chains, unsigned nb, unsigned seg, int floor_mode);
int launch_vorbis_coupling(symaccel_ctx *ctx, float *d_mag, float *d_ang, size_t n);
int launch_vorbis_prepare(symaccel_ctx *ctx, float *d_residue, size_t spec_stride, unsigned channels_per_stream, size_t n_streams,
                          size_t blocks, const uint32_t *d_block_off, const uint8_t *d_steps, const uint32_t *d_step_first,
                          const uint8_t *d_kill);
int launch_vorbis_dot(symaccel_ctx *ctx, float *d_floor, const float *d_residue, size_t total);
int launch_vorbis_deinterleave(symaccel_ctx *ctx, const float *d_type2, float *d_planar, int n_ch, size_t n2,
                               size_t count);
int launch_vorbis_floor1(symaccel_ctx *ctx, const uint32_t *h_setup, int n_posts, int multiplier,
                         const uint32_t *d_y, uint32_t n, float *d_floor, size_t count, const float *d_residue = nullptr,
                         uint8_t *d_floor_y = nullptr, const uint32_t *d_line_offs = nullptr);
int launch_vorbis_floor1_pair(symaccel_ctx *ctx, const uint32_t *const h_setup[2], const int n_posts[2], const int multiplier[2],
                              const uint32_t *const d_y[2], const uint32_t n[2], const size_t count[2], const uint32_t *const d_line_offs[2],
                              uint8_t *d_floor_y);
int launch_aac_joint_stereo(symaccel_ctx *ctx, const AacBandMaps &maps, float *d_coeffs, size_t frames_per_chain,
                            const int32_t *d_pair_chains, const symaccel_aac_js_frame *d_desc, size_t n_pairs,
                            const uint32_t *d_list = nullptr, size_t n_list = 0);
int launch_aac_js_consume(symaccel_ctx *ctx, symaccel_aac_js_frame *d_desc, const uint32_t *d_list, size_t n_list, size_t n_pair_frames);
bool aac_band_maps(const uint16_t *swb_long, int n_swb_long, const uint16_t *swb_short, int n_swb_short, AacBandMaps *maps);
int launch_aac_tns(symaccel_ctx *ctx, float *d_coeffs, size_t n_frames, const symaccel_aac_tns_filter *d_filters,
                   size_t n_filters);
int launch_mp3_decode(symaccel_ctx *ctx, const int16_t *d_quant, const symaccel_mp3_requant *d_rq_desc, const int32_t *d_pair_chains,
                      const symaccel_mp3_stereo *d_st_desc, size_t n_pairs, const symaccel_mp3_side *d_side, int sr,
                      const float *d_overlap_in, const float *d_vvec_in, const int32_t *d_vfront_in, float *d_overlap_out,
                      float *d_vvec_out, int32_t *d_vfront_out, float *d_pcm, size_t n_chains, size_t granules_per_chain);
int launch_mp3_stereo(symaccel_ctx *ctx, float *d_xr, size_t granules_per_chain, const int32_t *d_pair_chains,
                      const symaccel_mp3_stereo *d_desc, int sr, size_t n_pairs, const int16_t *d_quant = nullptr,
                      const symaccel_mp3_requant *d_rq_desc = nullptr);
int launch_mp3_requantize(symaccel_ctx *ctx, const int16_t *d_quant, const symaccel_mp3_requant *d_desc, int sr,
                          float *d_xr, size_t n);
int launch_mpa_polyphase(symaccel_ctx *ctx, int n_frames, const float *d_in, const float *d_vvec_in,
                         const int32_t *d_vfront_in, float *d_vvec_out, int32_t *d_vfront_out, float *d_pcm, size_t n_chains,
                         size_t packets_per_chain);
// mpa_polyphase.hip, the fused form: codes + records in, dequantised on load (d_status may be null)
int launch_mpa12_decode(symaccel_ctx *ctx, int layer, const uint16_t *d_codes, const uint8_t *d_rec, uint8_t *d_status,
                        const float *d_vvec_in, const int32_t *d_vfront_in, float *d_vvec_out, int32_t *d_vfront_out, float *d_pcm,
                        size_t n_chains, size_t packets_per_chain);
int launch_alac_predict(symaccel_ctx *ctx, int32_t *d_buf, const symaccel_alac_desc *d_desc, const int32_t *d_coeffs,
                        size_t n_blocks, size_t blocksize, const int32_t *d_pair_weight = nullptr,
                        const uint8_t *d_pair_shift = nullptr, size_t stride = 0 /* words between rows; 0 = blocksize */);
int launch_alac_mid_side(symaccel_ctx *ctx, const int32_t *d_weight, const uint8_t *d_shift, int32_t *d_ch0, int32_t *d_ch1,
                         size_t n_pairs, size_t blocksize);
int launch_state_copy(symaccel_ctx *ctx, void *dst0, const void *src0, size_t bytes0, void *dst1, const void *src1,
                      size_t bytes1, void *dst2, const void *src2, size_t bytes2);
int launch_flac_status(symaccel_ctx *ctx, const symaccel_flac_desc *d_desc, size_t n, size_t blocksize, int8_t *d_status);
int launch_alac_status(symaccel_ctx *ctx, const symaccel_alac_desc *d_desc, size_t n, int8_t *d_status);
int launch_floor1_status(symaccel_ctx *ctx, const uint32_t *d_y, size_t count, int n_posts, int8_t *d_status);
int launch_tns_status(symaccel_ctx *ctx, const symaccel_aac_tns_filter *d_filters, size_t n, size_t n_frames, int8_t *d_status);
// symaccel_row_stride() pads rows that are a multiple of 2 KiB long (1024 samples and more) by this fraction of the row; the sweeps behind it:
// profiles/r06zz30_stride_sweep.txt, r06zz31_stride_sweep.txt
constexpr size_t kRowPadDiv = 8;
int launch_flac_restore(symaccel_ctx *ctx, int32_t *d_buf, const symaccel_flac_desc *d_desc,
                        const int32_t *d_coeffs, size_t n_blocks, size_t blocksize, const uint8_t *d_pair_mode = nullptr,
                        uint32_t out_shift = 0, size_t stride = 0 /* words between rows; 0 = blocksize */);
// batch_copy.hip: one piece (<= kBatchCopyPiece bytes) per workgroup, host (page-locked) <-> device in either direction
// `pad` 0: copy `bytes` bytes.  Otherwise a CONVERTING piece of a scatter (a ticket with an output format): kBatchPieceConvert | kBatchPieceFromI32
// (the planes hold i32, else f32) | frames << 12 (at most 4096) | channels << 8 | the destination SYMACCEL_FMT_*; src = the piece's first frame in the
// first plane of its interleave group, the other planes launch_batch_copy's pcm_plane_stride samples apart; dst / bytes = its interleaved output
struct BatchCopyDesc {
    const void *src;
    void *dst;
    uint32_t bytes, pad;
};
constexpr size_t kBatchCopyPiece = 16384;
constexpr uint32_t kBatchPieceConvert = 0x80000000u, kBatchPieceFromI32 = 0x10u;
// A WIDENING piece of a gather (a ticket whose plane 0 came as int16_t, symaccel_batcher_reserve_io): src = int16_t words in the slot, dst =
// int32_t words on the device, bytes = the destination's.  A bit the converting pieces' encoding leaves alone; launch_batch_copy's `widening`
// says that a gather's list holds such pieces.
constexpr uint32_t kBatchPieceWiden = 0x40000000u;
// ... and beside it the width of the source's words where it is not 2: a row of a ticket that came with a width per row
// (SYMACCEL_IN_FMT_ROWS) at 3 bytes a word -- little-endian two's-complement, packed, src 4-byte aligned.  (A row at 4 bytes is a plain piece.)
constexpr uint32_t kBatchPiecePacked24 = 0x20000000u;
constexpr uint32_t batch_piece_widen(unsigned word_bytes) { return kBatchPieceWiden | (word_bytes == 3 ? kBatchPiecePacked24 : 0u); }
constexpr uint32_t batch_piece_convert(bool from_i32, size_t frames, uint32_t channels, int dst_fmt) {  // the `pad` word of a converting piece
    return kBatchPieceConvert | (from_i32 ? kBatchPieceFromI32 : 0u) | ((uint32_t)frames << 12) | (channels << 8) | (uint32_t)dst_fmt;
}
int launch_batch_copy(symaccel_ctx *ctx, hipStream_t stream, const BatchCopyDesc *descs, size_t n, bool scatter, size_t pcm_plane_stride = 0,
                      bool widening = false);
int launch_batch_flag(symaccel_ctx *ctx, hipStream_t stream, uint64_t *h_flag, uint64_t seq);  // (h_flag: page-locked host memory)
// pcm_convert.h works in tiles: a frame range of one interleave group whose output is contiguous and at most kPcmTileBytes long (the piece
// size of the batcher's scatter).  Frames of a tile: a multiple of 16 (so every tile of a group starts at the group's alignment modulo 16
// bytes), at most 4096.
constexpr unsigned kPcmTileBytes = 16384;
constexpr unsigned kPcmMaxChannels = 8;
constexpr unsigned pcm_tile_frames(unsigned channels, unsigned sample_bytes) {
    const unsigned f = (kPcmTileBytes / (channels * sample_bytes)) & ~15u;
    return f > 4096u ? 4096u : f;
}
// batch_copy.hip: planes of F32 / S32 samples to interleaved samples of dst_fmt (pcm_convert.h); arguments as symaccel_pcm_convert_device, already checked
int launch_pcm_convert(symaccel_ctx *ctx, hipStream_t stream, const void *d_src, int src_fmt, size_t plane_stride, size_t n_groups, size_t channels,
                       size_t n_frames, void *d_dst, int dst_fmt, size_t dst_group_bytes);
// what symaccel_pcm_convert(_device) refuse, pointers aside
inline bool pcm_convert_shape_ok(int src_fmt, size_t plane_stride, size_t n_groups, size_t channels, size_t n_frames, int dst_fmt, size_t dst_group_bytes) {
    const size_t b = symaccel_sample_bytes(dst_fmt);
    if ((src_fmt != SYMACCEL_FMT_F32 && src_fmt != SYMACCEL_FMT_S32) || b == 0 || channels < 1 || channels > 8) return false;
    if (n_frames > (size_t)1 << 36 || plane_stride > (size_t)1 << 36 || n_groups > (size_t)1 << 20 || dst_group_bytes > (size_t)1 << 40) return false;  // (keeps the extents in 64 bits)
    if (plane_stride < n_frames || dst_group_bytes < n_frames * channels * b) return false;
    return !((b == 2 || b == 4) && dst_group_bytes % b != 0);
}
// adpcm.hip: bytes of one block (symphonia-codec-adpcm: codec_ms.rs:101-136, codec_ima_wav.rs:27-65, codec_ima_qt.rs:24-47), 0 for the
// shapes the device decoder refuses: those where the reference leaves samples of a block unwritten or indexes out of range (MS with
// fewer than 2 frames or a mono block of odd length, IMA WAV mono of even length, IMA WAV stereo unless (fpb - 1) % 8 == 0, IMA QT other
// than 64 frames), more than two channels (lib.rs:97-99), and more than kAdpcmMaxFrames frames (keeps a block's offsets in 32 bits)
constexpr size_t kAdpcmMaxFrames = (size_t)1 << 20;
inline size_t adpcm_block_bytes(int codec, size_t channels, size_t fpb) {
    if ((channels != 1 && channels != 2) || fpb == 0 || fpb > kAdpcmMaxFrames) return 0;
    switch (codec) {
    case SYMACCEL_ADPCM_MS:
        if (fpb < 2 || (channels == 1 && fpb % 2 != 0)) return 0;
        return channels == 1 ? 6 + fpb / 2 : 12 + fpb;
    case SYMACCEL_ADPCM_IMA_WAV:
        if (channels == 1) return fpb % 2 == 0 ? 0 : 4 + (fpb - 1) / 2;
        return (fpb - 1) % 8 != 0 ? 0 : 7 + fpb;
    case SYMACCEL_ADPCM_IMA_QT: return fpb != 64 ? 0 : 34 * channels;
    default: return 0;
    }
}
// the frames of a block of `bytes` bytes (the inverse of the table above), 0 if no accepted shape has that many
inline size_t adpcm_frames_of_bytes(int codec, size_t channels, size_t bytes) {
    size_t fpb = 0;
    switch (codec) {
    case SYMACCEL_ADPCM_MS: fpb = channels == 1 ? (bytes >= 7 ? 2 * (bytes - 6) : 0) : (bytes >= 14 ? bytes - 12 : 0); break;
    case SYMACCEL_ADPCM_IMA_WAV: fpb = channels == 1 ? (bytes >= 4 ? 2 * (bytes - 4) + 1 : 0) : (bytes >= 8 ? bytes - 7 : 0); break;
    case SYMACCEL_ADPCM_IMA_QT: fpb = 64; break;
    default: break;
    }
    return fpb != 0 && adpcm_block_bytes(codec, channels, fpb) == bytes ? fpb : 0;
}
// what symaccel_adpcm_decode(_device) refuse, pointers aside: SYMACCEL_OK, or the error
inline int adpcm_shape_status(size_t block_pitch, size_t n_blocks, int codec, size_t channels, size_t fpb, int out_fmt) {
    if (codec != SYMACCEL_ADPCM_MS && codec != SYMACCEL_ADPCM_IMA_WAV && codec != SYMACCEL_ADPCM_IMA_QT) return SYMACCEL_ERR_INVALID_ARG;
    if (out_fmt != 0 && symaccel_sample_bytes(out_fmt) == 0) return SYMACCEL_ERR_INVALID_ARG;
    if (n_blocks > (size_t)1 << 32 || block_pitch > (size_t)1 << 24) return SYMACCEL_ERR_INVALID_ARG;
    const size_t bytes = adpcm_block_bytes(codec, channels, fpb);
    if (bytes == 0) return SYMACCEL_ERR_UNSUPPORTED;
    return block_pitch < bytes ? SYMACCEL_ERR_INVALID_ARG : SYMACCEL_OK;
}
int launch_adpcm_decode(symaccel_ctx *ctx, hipStream_t stream, const void *d_bytes, size_t block_pitch, size_t n_blocks, int codec, unsigned channels,
                        unsigned frames_per_block, void *d_pcm, int out_fmt, uint8_t *d_status);
// pcm_decode.hip: what a SYMACCEL_PCM_* codec is (symphonia-codec-pcm lib.rs:248-262, 328-388)
enum PcmKind { PCM_KIND_SIGNED, PCM_KIND_UNSIGNED, PCM_KIND_F32, PCM_KIND_F64, PCM_KIND_ALAW, PCM_KIND_MULAW };
struct PcmCodec {
    unsigned coded;   // bytes of a coded sample: 1, 2, 3, 4, 8; 0 = an unknown codec
    unsigned native;  // bytes of a sample of the reference's buffer as Rust holds it: 1, 2, 4 (i24 / u24 are a u32 / i32 word), 8
    unsigned width;   // bits of the buffer's sample format (sample_format_width)
    PcmKind kind;
    bool big_endian;
};
inline PcmCodec pcm_codec(int codec) {
    switch (codec) {
    case SYMACCEL_PCM_S32LE: return {4, 4, 32, PCM_KIND_SIGNED, false};
    case SYMACCEL_PCM_S32BE: return {4, 4, 32, PCM_KIND_SIGNED, true};
    case SYMACCEL_PCM_S24LE: return {3, 4, 24, PCM_KIND_SIGNED, false};
    case SYMACCEL_PCM_S24BE: return {3, 4, 24, PCM_KIND_SIGNED, true};
    case SYMACCEL_PCM_S16LE: return {2, 2, 16, PCM_KIND_SIGNED, false};
    case SYMACCEL_PCM_S16BE: return {2, 2, 16, PCM_KIND_SIGNED, true};
    case SYMACCEL_PCM_S8: return {1, 1, 8, PCM_KIND_SIGNED, false};
    case SYMACCEL_PCM_U32LE: return {4, 4, 32, PCM_KIND_UNSIGNED, false};
    case SYMACCEL_PCM_U32BE: return {4, 4, 32, PCM_KIND_UNSIGNED, true};
    case SYMACCEL_PCM_U24LE: return {3, 4, 24, PCM_KIND_UNSIGNED, false};
    case SYMACCEL_PCM_U24BE: return {3, 4, 24, PCM_KIND_UNSIGNED, true};
    case SYMACCEL_PCM_U16LE: return {2, 2, 16, PCM_KIND_UNSIGNED, false};
    case SYMACCEL_PCM_U16BE: return {2, 2, 16, PCM_KIND_UNSIGNED, true};
    case SYMACCEL_PCM_U8: return {1, 1, 8, PCM_KIND_UNSIGNED, false};
    case SYMACCEL_PCM_F32LE: return {4, 4, 32, PCM_KIND_F32, false};
    case SYMACCEL_PCM_F32BE: return {4, 4, 32, PCM_KIND_F32, true};
    case SYMACCEL_PCM_F64LE: return {8, 8, 64, PCM_KIND_F64, false};
    case SYMACCEL_PCM_F64BE: return {8, 8, 64, PCM_KIND_F64, true};
    case SYMACCEL_PCM_ALAW: return {1, 2, 16, PCM_KIND_ALAW, false};
    case SYMACCEL_PCM_MULAW: return {1, 2, 16, PCM_KIND_MULAW, false};
    default: return {0, 0, 0, PCM_KIND_SIGNED, false};
    }
}
// The extents symaccel_pcm_decode(_device) accept: they keep every byte offset below 2^62
constexpr size_t kPcmDecMaxPackets = (size_t)1 << 32, kPcmDecMaxFrames = (size_t)1 << 36, kPcmDecMaxPitch = (size_t)1 << 40, kPcmDecMaxBytes = (size_t)1 << 62;
// what symaccel_pcm_decode(_device) refuse, pointers aside: SYMACCEL_OK, or the error.  UNSUPPORTED is what the reference's decoder takes
// and this one leaves to it (lib.rs:231-241 any channel count; :307 a coded width of 0, where `<<` by the whole width overflows; a
// shift on the codecs whose widths :292-303 pin, which try_new never produces)
inline int pcm_decode_shape_status(size_t packet_pitch, size_t n_packets, int codec, size_t channels, unsigned shift, size_t frames, int out_fmt) {
    const PcmCodec pc = pcm_codec(codec);
    if (pc.coded == 0 || (out_fmt != 0 && symaccel_sample_bytes(out_fmt) == 0)) return SYMACCEL_ERR_INVALID_ARG;
    if (channels < 1 || channels > kPcmMaxChannels) return SYMACCEL_ERR_UNSUPPORTED;
    const bool integer = pc.kind == PCM_KIND_SIGNED || pc.kind == PCM_KIND_UNSIGNED;
    if (integer ? shift == pc.width : shift != 0) return SYMACCEL_ERR_UNSUPPORTED;
    if (shift > pc.width) return SYMACCEL_ERR_INVALID_ARG;
    if (n_packets > kPcmDecMaxPackets || frames > kPcmDecMaxFrames || packet_pitch > kPcmDecMaxPitch) return SYMACCEL_ERR_INVALID_ARG;
    if (packet_pitch < frames * channels * pc.coded) return SYMACCEL_ERR_INVALID_ARG;
    const size_t per_packet = std::max<size_t>(packet_pitch, frames * channels * 8);
    if (n_packets != 0 && per_packet > kPcmDecMaxBytes / n_packets) return SYMACCEL_ERR_INVALID_ARG;
    return SYMACCEL_OK;
}
// Frames of a tile of pcm_decode.hip: a multiple of 16, with the tile's coded bytes and its output (and the up to 31 bytes of alignment
// slack of each of its up to 8 output runs) inside kPcmTileBytes
constexpr unsigned pcm_decode_tile_frames(unsigned channels, unsigned coded_bytes, unsigned out_bytes) {
    return ((kPcmTileBytes - 256u) / (channels * (coded_bytes > out_bytes ? coded_bytes : out_bytes))) & ~15u;
}
// (the caller has checked the shape, the pointers' alignment and the sizes: symaccel_pcm_decode_device)
int launch_pcm_decode(symaccel_ctx *ctx, hipStream_t stream, const void *d_bytes, size_t packet_pitch, size_t n_packets, int codec, unsigned channels,
                      unsigned shift, size_t frames, void *d_pcm, int out_fmt);
int launch_probe_copy(symaccel_ctx *ctx, const void *d_src, void *d_dst, size_t bytes, unsigned frames_per_wavefront, unsigned flags);
int launch_flac_decorrelate(symaccel_ctx *ctx, const uint8_t *d_mode, int32_t *d_ch0, int32_t *d_ch1,
                            size_t n_pairs, size_t blocksize, uint32_t out_shift);
// flac.hip: STREAMINFO MD5, one lane per job (d_jobs and everything it points to on the device)
int launch_flac_md5(symaccel_ctx *ctx, const symaccel_flac_md5_job *d_jobs, size_t n_jobs, bool finish = false, uint32_t out_shift = 0);

}  // namespace symaccel
