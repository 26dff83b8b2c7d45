// symaccel.hpp -- C++17 host-side mirror of the reference's DSP interfaces on top of the symaccel C ABI.
//
// The reference (pdeljanov/Symphonia 0.6.1) is Rust; this image has no Rust toolchain, so the host side
// above the C ABI is written in C++ (and, for the tests / bench harness, in Python: symphonia_amd/).  Every
// type below mirrors one reference item -- same name, same argument meaning, same error behaviour:
//
//   dsp::mdct::Imdct           symphonia-core/src/dsp/mdct.rs:16-146
//   dsp::fft::Fft              symphonia-core/src/dsp/fft/no_simd.rs:70-141
//   aac::Dsp                   symphonia-codec-aac/src/aac/dsp.rs:22-158
//   mp3::SynthesisState, mp3::GranuleChannel, mp3::synthesize_granule
//                              symphonia-bundle-mp3/src/synthesis.rs:145-336, layer3/hybrid_synthesis.rs:153-485,
//                              the per-channel tail of Layer3::decode (layer3/mod.rs:440-476)
//   vorbis::Windows / Dsp / DspChannel   symphonia-codec-vorbis/src/dsp.rs:12-145, window.rs:11-39
//   flac::lpc_predict / fixed_predict / decorrelate_*   symphonia-bundle-flac/src/decoder.rs:32-82, 663-752
//   alac::ElementChannel::predict / decorrelate_mid_side   symphonia-codec-alac/src/lib.rs:165-264, 664-671
//
// Error behaviour: what the reference asserts / panics on (slice lengths, non power-of-two sizes) throws
// std::invalid_argument; what it would return as Error::Unsupported throws Error{Kind::Unsupported}; HIP /
// device / allocation failures throw Error{Kind::IoError} (symphonia-core/src/errors.rs:38-54).  There is no
// CPU fallback: constructing a Context without an MI355X throws.
//
// The per-packet calls here are batches of one and are latency-bound by design (one launch + PCIe round trip
// per call); the *_batch members are the path the GPU is for.
#ifndef SYMACCEL_HPP
#define SYMACCEL_HPP

#include <array>
#include <algorithm>
#include <complex>
#include <functional>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <optional>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <cstring>
#include <typeindex>
#include <vector>

#include "symaccel.h"

namespace symphonia_accel {

class Error : public std::runtime_error {
public:
    enum class Kind { IoError, Unsupported };  // errors.rs:38-54
    Error(Kind k, int status, const std::string &what) : std::runtime_error(what), kind(k), status(status) {}
    Kind kind;
    int status;
};

inline void check(int status, const symaccel_ctx *ctx = nullptr) {
    if (status >= 0) return;
    std::string msg = symaccel_strerror(status);
    if (ctx) {
        const char *extra = symaccel_last_error(ctx);
        if (extra && *extra) msg += std::string(": ") + extra;
    }
    if (status == SYMACCEL_ERR_INVALID_ARG) throw std::invalid_argument(msg);  // the reference's assert!/panic class
    throw Error(status == SYMACCEL_ERR_UNSUPPORTED ? Error::Kind::Unsupported : Error::Kind::IoError, status, msg);
}

// The sample formats PCM can be delivered in (SYMACCEL_FMT_*; symphonia-core/src/audio/sample.rs: u8 .. f32, the 24-bit ones as three packed
// little-endian bytes).  Native = the planes as the decoders leave them: planar f32, or left-justified i32 for FLAC.
enum class SampleFormat : int {
    Native = 0,
    U8 = SYMACCEL_FMT_U8,
    S8 = SYMACCEL_FMT_S8,
    U16 = SYMACCEL_FMT_U16,
    S16 = SYMACCEL_FMT_S16,
    U24 = SYMACCEL_FMT_U24,
    S24 = SYMACCEL_FMT_S24,
    U32 = SYMACCEL_FMT_U32,
    S32 = SYMACCEL_FMT_S32,
    F32 = SYMACCEL_FMT_F32
};
inline std::size_t sample_bytes(SampleFormat f) { return symaccel_sample_bytes(static_cast<int>(f)); }

// One context = one HIP device + stream + device-resident constant tables.  Externally synchronised, like
// `&mut self` on the reference's decoders; distinct contexts may be used from distinct threads.
class Context {
public:
    explicit Context(int device = 0) { check(symaccel_ctx_create(device, &ctx_)); }
    ~Context() {
        if (ctx_) symaccel_ctx_destroy(ctx_);
    }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    Context(Context &&o) noexcept : ctx_(std::exchange(o.ctx_, nullptr)) {}
    symaccel_ctx *raw() const { return ctx_; }
    void sync() { check(symaccel_sync(ctx_), ctx_); }
    void set_segment(int frames) { check(symaccel_ctx_set_segment(ctx_, frames), ctx_); }
    // GenericAudioBufferRef::copy_bytes_to_vec_interleaved_as::<S> (audio/generic.rs:204-340) for planes in host memory: n_groups groups of
    // `channels` planes (F32 or S32, plane_stride samples apart, n_frames valid) to [n_frames][channels] samples of `dst` per group,
    // dst_group_bytes apart -- FromSample (audio/conv.rs) and the interleave (audio/util.rs:119-167) on the device
    void pcm_convert(const void *h_src, SampleFormat src, std::size_t plane_stride, std::size_t n_groups, std::size_t channels, std::size_t n_frames, void *h_dst,
                     SampleFormat dst, std::size_t dst_group_bytes) {
        check(symaccel_pcm_convert(ctx_, h_src, static_cast<int>(src), plane_stride, n_groups, channels, n_frames, h_dst, static_cast<int>(dst), dst_group_bytes), ctx_);
    }
    // symphonia-codec-adpcm's block decoders (codec_ms.rs, codec_ima_wav.rs, codec_ima_qt.rs) for n_blocks blocks in host memory,
    // block_pitch bytes apart: h_pcm[n_blocks][channels][frames_per_block] i32 (Native), or [n_blocks][frames_per_block][channels] samples
    // of `out`; h_status[n_blocks] (may be null): 0, 1 = MS block predictor out of range, 2 = IMA WAV step index out of range
    void adpcm_decode(const void *h_bytes, std::size_t block_pitch, std::size_t n_blocks, int codec, std::size_t channels, std::size_t frames_per_block, void *h_pcm,
                      SampleFormat out = SampleFormat::Native, std::uint8_t *h_status = nullptr) {
        check(symaccel_adpcm_decode(ctx_, h_bytes, block_pitch, n_blocks, codec, channels, frames_per_block, h_pcm, static_cast<int>(out), h_status), ctx_);
    }
    // symphonia-codec-pcm's PcmDecoder::decode_inner (lib.rs:318-411) for n_packets packets of `frames` frames in host memory,
    // packet_pitch bytes apart; codec: SYMACCEL_PCM_*; shift: bits_per_sample - bits_per_coded_sample (lib.rs:307).
    // h_pcm[n_packets][channels][frames] native samples (symaccel_pcm_native_bytes each), or [n_packets][frames][channels] samples of `out`
    void pcm_decode(const void *h_bytes, std::size_t packet_pitch, std::size_t n_packets, int codec, std::size_t channels, std::uint32_t shift, std::size_t frames,
                    void *h_pcm, SampleFormat out = SampleFormat::Native) {
        check(symaccel_pcm_decode(ctx_, h_bytes, packet_pitch, n_packets, codec, channels, shift, frames, h_pcm, static_cast<int>(out)), ctx_);
    }
    // Layer1::decode / Layer2::decode behind the bit reader (layer1/mod.rs:142-194, layer2/mod.rs:320-384) for n_chains x
    // packets_per_chain channel-packets in host memory: h_codes[chain][packet][32][n_frames] u16, h_rec[chain][packet][record bytes],
    // state and PCM as mp3::synthesis takes them; h_status[chain][packet] (may be null): 1 = a record out of range, decoded as silence
    void mpa12_decode(int layer, const std::uint16_t *h_codes, const std::uint8_t *h_rec, float *h_vvec_io, std::int32_t *h_vfront_io, float *h_pcm,
                      std::size_t n_chains, std::size_t packets_per_chain, std::uint8_t *h_status = nullptr) {
        check(symaccel_mpa12_decode(ctx_, layer, h_codes, h_rec, h_vvec_io, h_vfront_io, h_pcm, h_status, n_chains, packets_per_chain), ctx_);
    }

private:
    symaccel_ctx *ctx_ = nullptr;
};

// The cross-stream batcher (symaccel_batcher_*, csrc/batcher.cpp): one per process and context, shared by every decoder of the
// process.  Decoders submit their look-ahead batches; one launch per (kind, units) group serves all of them.  Thread-safe.
class Batcher {
public:
    explicit Batcher(Context &ctx, std::size_t flush_bytes = 0) : ctx_(ctx) {
        check(symaccel_batcher_create(ctx.raw(), flush_bytes, &b_), ctx.raw());
        if (const char *e = std::getenv("SYMACCEL_NARROW_INPUT")) {  // (read once, like the library's own batcher knobs)
            const int v = std::atoi(e);
            input_mode_ = v == 2 ? InputMode::Rows : v != 0 ? InputMode::NarrowBatches : InputMode::Wide;
        }
    }
    ~Batcher() {
        if (b_) symaccel_batcher_destroy(b_);
    }
    Batcher(const Batcher &) = delete;
    Batcher &operator=(const Batcher &) = delete;
    symaccel_batcher *raw() const { return b_; }
    Context &context() const { return ctx_; }
    void flush() { check(symaccel_batcher_flush(b_), ctx_.raw()); }
    void hint() { check(symaccel_batcher_hint(b_), ctx_.raw()); }
    symaccel_batcher_stats stats() const {
        symaccel_batcher_stats s{};
        check(symaccel_batcher_get_stats(b_, &s), ctx_.raw());
        return s;
    }
    // symaccel_batcher_reserve_io: a slot whose plane 0 takes int16_t words (in_fmt SYMACCEL_FMT_S16; FLAC_RESTORE / ALAC_PREDICT), widened in
    // the gather of the launch; in_fmt SYMACCEL_IN_FMT_ROWS: every row of plane 0 at its native offset at 2, 3 or 4 bytes a word, the widths in
    // slot->input[5]; in_fmt 0 = the native planes.  out_fmt / channels as symaccel_batcher_reserve_fmt takes them (0 = native).
    void reserve_io(int kind, int param, std::size_t n_chains, std::size_t units_per_chain, int in_fmt, int out_fmt, int channels, symaccel_batch_slot *slot,
                    std::uint64_t *ticket) {
        check(symaccel_batcher_reserve_io(b_, kind, param, n_chains, units_per_chain, in_fmt, out_fmt, channels, slot, ticket), ctx_.raw());
    }
    // How the FLAC decoders on this batcher send plane 0 up; read by a decoder when it attaches.  SYMACCEL_NARROW_INPUT when the batcher is
    // made, or the setters: unset or 0 = Wide, every batch as int32_t, as it always was; 1 = NarrowBatches (set_narrow_input(true)), a batch
    // whose every word fits int16_t goes as int16_t and any other wide; 2 = Rows, every row (subframe) at the narrowest of 2, 3 or 4 bytes a
    // word that holds it (SYMACCEL_IN_FMT_ROWS), decided while the slot is filled, with no pass over the batch in front.
    enum class InputMode { Wide = 0, NarrowBatches = 1, Rows = 2 };
    InputMode input_mode() const { return input_mode_; }
    void set_input_mode(InputMode m) { input_mode_ = m; }
    bool narrow_input() const { return input_mode_ == InputMode::NarrowBatches; }
    void set_narrow_input(bool on) { input_mode_ = on ? InputMode::NarrowBatches : InputMode::Wide; }
    // The process-wide batcher (the Rust shim's Pool::shared(), bindings/rust/symphonia-accel-hip/src/ctx.rs): device 0, the library's
    // default flush size, created on first use and never destroyed (decoders of any thread may hold it until the process ends).  This is
    // what a factory that sees (params, options) alone -- CodecRegistry::make_audio_decoder below, registry.rs:330-341 -- builds through.
    // Throws what Context / Batcher construction throws (no device: Error{IoError}); a failed first attempt is not retried.
    static Batcher &shared() {
        static std::once_flag once;
        static Batcher *inst = nullptr;
        static std::string failure;
        std::call_once(once, [] {
            try {
                auto *ctx = new Context(0);
                try {
                    inst = new Batcher(*ctx, 0);
                } catch (...) {
                    delete ctx;
                    throw;
                }
            } catch (const std::exception &e) {
                failure = e.what();
            }
        });
        if (!inst) throw Error(Error::Kind::IoError, SYMACCEL_ERR_DEVICE, "shared batcher: " + failure);
        return *inst;
    }

private:
    Context &ctx_;
    symaccel_batcher *b_ = nullptr;
    InputMode input_mode_ = InputMode::Wide;
};

namespace dsp {
namespace mdct {

// Imdct (mdct.rs:16-20): N spectral lines in, 2N samples out.
class Imdct {
public:
    // Imdct::new(n) (mdct.rs:27-29)
    Imdct(Context &ctx, std::size_t n) : Imdct(ctx, n, 1.0) {}
    // Imdct::new_scaled(n, scale) (mdct.rs:35-60); panics unless n is a power of two (mdct.rs:37-40)
    static Imdct new_scaled(Context &ctx, std::size_t n, double scale) { return Imdct(ctx, n, scale); }

    // imdct(&mut self, spec: &[f32], out: &mut [f32]) (mdct.rs:67-146); asserts spec.len() == n, out.len() == 2n
    void imdct(const float *spec, std::size_t spec_len, float *out, std::size_t out_len) {
        if (spec_len != n_ || out_len != 2 * n_) throw std::invalid_argument("Imdct::imdct: slice lengths (mdct.rs:76-78)");
        check(symaccel_imdct_f32(ctx_.raw(), (int)n_, scale_, spec, out, 1), ctx_.raw());
    }
    // `count` transforms back to back: spec[count][n] -> out[count][2n]
    void imdct_batch(const float *spec, float *out, std::size_t count) {
        check(symaccel_imdct_f32(ctx_.raw(), (int)n_, scale_, spec, out, count), ctx_.raw());
    }

private:
    Imdct(Context &ctx, std::size_t n, double scale) : ctx_(ctx), n_(n), scale_(scale) {
        if (n < 4 || (n & (n - 1)) != 0) throw std::invalid_argument("Imdct: n must be a power of two (mdct.rs:37)");
        if (n > 8192) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "Imdct: n > 8192");
    }
    Context &ctx_;
    std::size_t n_;
    double scale_;
};

}  // namespace mdct

namespace fft {

using Complex = std::complex<float>;  // num_complex::Complex<f32>, same (re, im) layout

// Fft (no_simd.rs:70-141).  MAX_SIZE is the reference's (1 << 16: its permutation table is u16).
class Fft {
public:
    static constexpr std::size_t MAX_SIZE = 65536;
    Fft(Context &ctx, std::size_t n) : ctx_(ctx), n_(n) {
        if (n < 2 || (n & (n - 1)) != 0) throw std::invalid_argument("Fft: n must be a power of two (no_simd.rs:77)");
        if (n > MAX_SIZE) throw std::invalid_argument("Fft: n > MAX_SIZE (no_simd.rs:80)");
    }
    std::size_t size() const { return n_; }
    // fft_inplace(&mut self, x: &mut [Complex<f32>]) (no_simd.rs:96-118)
    void fft_inplace(Complex *x, std::size_t len) {
        if (len != n_) throw std::invalid_argument("Fft::fft_inplace: slice length (no_simd.rs:97)");
        check(symaccel_fft_c32(ctx_.raw(), (int)n_, reinterpret_cast<const float *>(x), reinterpret_cast<float *>(x), 1),
              ctx_.raw());
    }
    // fft(&mut self, x: &[Complex<f32>], y: &mut [Complex<f32>]) (no_simd.rs:121-140)
    void fft(const Complex *x, std::size_t x_len, Complex *y, std::size_t y_len) {
        if (x_len != n_ || y_len != n_) throw std::invalid_argument("Fft::fft: slice lengths (no_simd.rs:122-123)");
        check(symaccel_fft_c32(ctx_.raw(), (int)n_, reinterpret_cast<const float *>(x), reinterpret_cast<float *>(y), 1),
              ctx_.raw());
    }

private:
    Context &ctx_;
    std::size_t n_;
};

// Ifft (no_simd.rs:143-219): the forward transform between a re <-> im swap on the way in and a swap with the 1 / n scale
// on the way out.  (As in the reference, fewer than 32 points only permute, swap and scale: its transform() has no case
// for them.)
class Ifft {
public:
    static constexpr std::size_t MAX_SIZE = 65536;
    Ifft(Context &ctx, std::size_t n) : ctx_(ctx), n_(n) {
        if (n < 2 || (n & (n - 1)) != 0) throw std::invalid_argument("Ifft: n must be a power of two (no_simd.rs:152)");
        if (n > MAX_SIZE) throw std::invalid_argument("Ifft: n > MAX_SIZE (no_simd.rs:155)");
    }
    std::size_t size() const { return n_; }
    // ifft_inplace(&mut self, x: &mut [Complex<f32>]) (no_simd.rs:189-218)
    void ifft_inplace(Complex *x, std::size_t len) {
        if (len != n_) throw std::invalid_argument("Ifft::ifft_inplace: slice length (no_simd.rs:191)");
        check(symaccel_ifft_c32(ctx_.raw(), (int)n_, reinterpret_cast<const float *>(x), reinterpret_cast<float *>(x), 1), ctx_.raw());
    }
    // ifft(&mut self, x: &[Complex<f32>], y: &mut [Complex<f32>]) (no_simd.rs:166-187)
    void ifft(const Complex *x, std::size_t x_len, Complex *y, std::size_t y_len) {
        if (x_len != n_ || y_len != n_) throw std::invalid_argument("Ifft::ifft: slice lengths (no_simd.rs:168-169)");
        check(symaccel_ifft_c32(ctx_.raw(), (int)n_, reinterpret_cast<const float *>(x), reinterpret_cast<float *>(y), 1), ctx_.raw());
    }

private:
    Context &ctx_;
    std::size_t n_;
};

}  // namespace fft
}  // namespace dsp

namespace aac {

// window sequences (aac/common.rs:17-20)
constexpr std::uint8_t ONLY_LONG_SEQUENCE = 0, LONG_START_SEQUENCE = 1, EIGHT_SHORT_SEQUENCE = 2, LONG_STOP_SEQUENCE = 3;

// aac::dsp::Dsp (aac/dsp.rs:22-158).  The windows, the two Imdcts and the scratch buffers of the reference's
// struct live in the context (device tables / LDS).
class Dsp {
public:
    explicit Dsp(Context &ctx) : ctx_(ctx) {}
    // synth(&mut self, coeffs: &[f32; 1024], delay: &mut [f32; 1024], seq: u8, window_shape: bool,
    //       prev_window_shape: bool, dst: &mut [f32])  (aac/dsp.rs:57-65)
    void synth(const std::array<float, 1024> &coeffs, std::array<float, 1024> &delay, std::uint8_t seq, bool window_shape,
               bool prev_window_shape, float *dst, std::size_t dst_len) {
        if (dst_len < 1024) throw std::invalid_argument("Dsp::synth: dst shorter than 1024 samples");
        const std::uint8_t side = SYMACCEL_AAC_SIDE(seq, window_shape ? 1u : 0u, prev_window_shape ? 1u : 0u);
        check(symaccel_aac_synth(ctx_.raw(), coeffs.data(), &side, delay.data(), dst, 1, 1), ctx_.raw());
    }
    // chain-major batch: coeffs[chain][frame][1024], side[chain][frame], delay[chain][1024], pcm[chain][frame][1024]
    void synth_batch(const float *coeffs, const std::uint8_t *side, float *delay_io, float *pcm, std::size_t n_chains,
                     std::size_t frames_per_chain) {
        check(symaccel_aac_synth(ctx_.raw(), coeffs, side, delay_io, pcm, n_chains, frames_per_chain), ctx_.raw());
    }

private:
    Context &ctx_;
};

// The stages between the spectrum decoder and Dsp::synth, batched and in place on DEVICE memory (the array
// Dsp::synth_batch's device twin consumes): joint-stereo decoding of ChannelPair::decode (aac/cpe.rs:110-157) and the
// filtering loops of Tns::synth (aac/ics/tns.rs:180-195).  Descriptors: see symaccel.h.
inline void joint_stereo_device(Context &ctx, float *d_coeffs, std::size_t frames_per_chain, const std::int32_t *d_pair_chains,
                                const symaccel_aac_js_frame *d_desc, std::size_t n_pairs, const std::vector<std::uint16_t> &swb_long,
                                const std::vector<std::uint16_t> &swb_short) {
    if (swb_long.size() < 2 || swb_short.size() < 2) throw std::invalid_argument("joint_stereo: swb offset tables");
    check(symaccel_aac_joint_stereo_device(ctx.raw(), d_coeffs, frames_per_chain, d_pair_chains, d_desc, n_pairs, swb_long.data(),
                                           (int)swb_long.size() - 1, swb_short.data(), (int)swb_short.size() - 1),
          ctx.raw());
}
inline void tns_device(Context &ctx, float *d_coeffs, std::size_t n_frames, const symaccel_aac_tns_filter *d_filters,
                       std::size_t n_filters) {
    check(symaccel_aac_tns_device(ctx.raw(), d_coeffs, n_frames, d_filters, n_filters), ctx.raw());
}

}  // namespace aac

namespace mp3 {

// BlockType (layer3/common.rs:174-185)
enum class BlockType : std::uint8_t { Long = 0, Start = 1, Short = 2, End = 3 };

// The GranuleChannel fields the synthesis tail reads (layer3/common.rs:187-230)
struct GranuleChannel {
    BlockType block_type = BlockType::Long;
    bool is_mixed = false;   // BlockType::Short { is_mixed }
    std::uint16_t rzero = 576;
};

// SynthesisState (synthesis.rs:145-154) plus the hybrid-synthesis overlap of one channel (layer3/mod.rs:258)
struct SynthesisState {
    std::array<float, 32 * 18> overlap{};
    std::array<float, 16 * 64> v_vec{};
    std::int32_t v_front = 0;
};

// One channel of one granule: reorder, antialias, hybrid_synthesis, frequency_inversion (hybrid_synthesis.rs:153-485)
// and synthesis::synthesis with n_frames = 18 (synthesis.rs:158-336).  samples = post requantize + stereo.
inline void synthesize_granule(Context &ctx, int sample_rate_idx, const GranuleChannel &gc, const std::array<float, 576> &samples,
                               SynthesisState &state, float *out, std::size_t out_len) {
    if (out_len < 576) throw std::invalid_argument("synthesize_granule: out shorter than 576 samples");
    const symaccel_mp3_side side{(std::uint8_t)gc.block_type, (std::uint8_t)(gc.is_mixed ? 1 : 0), gc.rzero};
    check(symaccel_mp3_synth(ctx.raw(), samples.data(), &side, sample_rate_idx, state.overlap.data(), state.v_vec.data(),
                             &state.v_front, out, 1, 1),
          ctx.raw());
}
inline void synthesize_batch(Context &ctx, int sample_rate_idx, const float *xr, const symaccel_mp3_side *side, float *overlap_io,
                             float *v_vec_io, std::int32_t *v_front_io, float *pcm, std::size_t n_chains,
                             std::size_t granules_per_chain) {
    check(symaccel_mp3_synth(ctx.raw(), xr, side, sample_rate_idx, overlap_io, v_vec_io, v_front_io, pcm, n_chains,
                             granules_per_chain),
          ctx.raw());
}

// requantize(header, channel, buf) (requantize.rs:356-380) together with the sample mapping of read_huffman_samples
// (requantize.rs:117-147): `quant` holds the signed quantised Huffman samples, `buf` receives xr.
struct RequantizeChannel {  // the GranuleChannel fields requantize reads (layer3/common.rs:187-230)
    std::uint8_t global_gain = 210;
    bool scalefac_scale = false, preflag = false;
    BlockType block_type = BlockType::Long;
    bool is_mixed = false;
    std::array<std::uint8_t, 3> subblock_gain{};
    std::uint16_t rzero = 576;
    std::array<std::uint8_t, 39> scalefacs{};
};
inline symaccel_mp3_requant to_abi(const RequantizeChannel &c) {
    symaccel_mp3_requant d{};
    d.global_gain = c.global_gain;
    d.flags = (std::uint8_t)((c.scalefac_scale ? SYMACCEL_MP3_RQ_SCALEFAC_SCALE : 0u) | (c.preflag ? SYMACCEL_MP3_RQ_PREFLAG : 0u));
    d.block_type = (std::uint8_t)c.block_type;
    d.is_mixed = c.is_mixed ? 1 : 0;
    for (int w = 0; w < 3; ++w) d.subblock_gain[w] = c.subblock_gain[(std::size_t)w];
    d.rzero = c.rzero;
    for (int i = 0; i < 39; ++i) d.scalefacs[i] = c.scalefacs[(std::size_t)i];
    return d;
}
inline void requantize(Context &ctx, int sample_rate_idx, const RequantizeChannel &channel, const std::array<std::int16_t, 576> &quant,
                       std::array<float, 576> &buf) {
    const symaccel_mp3_requant d = to_abi(channel);
    check(symaccel_mp3_requantize(ctx.raw(), quant.data(), &d, sample_rate_idx, buf.data(), 1), ctx.raw());
}
inline void requantize_batch(Context &ctx, int sample_rate_idx, const std::int16_t *quant, const symaccel_mp3_requant *desc, float *xr,
                             std::size_t n_granule_channels) {
    check(symaccel_mp3_requantize(ctx.raw(), quant, desc, sample_rate_idx, xr, n_granule_channels), ctx.raw());
}

// stereo(header, granule, ch) (stereo.rs:485-556), batched and in place on DEVICE memory: xr[chain][granule][576]
inline void stereo_device(Context &ctx, int sample_rate_idx, float *d_xr, std::size_t granules_per_chain,
                          const std::int32_t *d_pair_chains, const symaccel_mp3_stereo *d_desc, std::size_t n_pairs) {
    check(symaccel_mp3_stereo_device(ctx.raw(), d_xr, granules_per_chain, d_pair_chains, d_desc, sample_rate_idx, n_pairs), ctx.raw());
}

// synthesis(state, n_frames, in_samples, out) (synthesis.rs:158-336) as Layer I (n_frames 12) and Layer II (36) call it
inline void synthesis(Context &ctx, SynthesisState &state, std::size_t n_frames, const float *in_samples, std::size_t in_len,
                      float *out, std::size_t out_len) {
    if (in_len != 32 * n_frames || out_len < 32 * n_frames) throw std::invalid_argument("synthesis: slice lengths (synthesis.rs:162)");
    check(symaccel_mpa_polyphase(ctx.raw(), (int)n_frames, in_samples, state.v_vec.data(), &state.v_front, out, 1, 1), ctx.raw());
}

}  // namespace mp3

namespace vorbis {

// Dsp + DspChannel (vorbis/dsp.rs:12-66): block sizes, and per channel the overlap of the previous block.
class Dsp {
public:
    // bs0_exp / bs1_exp from the identification header (vorbis/lib.rs:404-406, 461-470)
    Dsp(Context &ctx, int bs0_exp, int bs1_exp) : ctx_(ctx), bs0_exp_(bs0_exp), bs1_exp_(bs1_exp) {
        if (bs0_exp < 6 || bs1_exp > 13 || bs0_exp > bs1_exp) throw std::invalid_argument("vorbis::Dsp: block sizes");
    }
    int bs0_exp() const { return bs0_exp_; }
    int bs1_exp() const { return bs1_exp_; }
    Context &context() { return ctx_; }

private:
    Context &ctx_;
    int bs0_exp_, bs1_exp_;
};

class DspChannel {
public:
    explicit DspChannel(Dsp &dsp) : dsp_(dsp), overlap_((std::size_t)1 << (dsp.bs1_exp() - 1), 0.0f) {}
    // reset (dsp.rs:128-132)
    void reset() { overlap_.assign(overlap_.size(), 0.0f); }
    // synth(&mut self, block_flag, prev_block_flag (lib.rs:298: None pairs the first block with itself), ..., buf)
    // spectrum = floor x residue, bs/2 values; returns the (prev_n + n) / 4 samples of lib.rs:303 in `out`.
    std::size_t synth(bool block_flag, std::optional<bool> prev_block_flag, const float *spectrum, float *out, std::size_t out_cap) {
        const int n = 1 << (block_flag ? dsp_.bs1_exp() : dsp_.bs0_exp());
        const bool pf = prev_block_flag.value_or(block_flag);
        const int prev_n = 1 << (pf ? dsp_.bs1_exp() : dsp_.bs0_exp());
        const std::size_t n_out = (std::size_t)(prev_n + n) / 4;
        if (out_cap < n_out) throw std::invalid_argument("DspChannel::synth: out too short");
        std::uint8_t flag = block_flag ? 1 : 0;
        std::int32_t pflag = prev_block_flag ? (*prev_block_flag ? 1 : 0) : -1;
        check(symaccel_vorbis_synth(dsp_.context().raw(), dsp_.bs0_exp(), dsp_.bs1_exp(), spectrum, (std::size_t)n / 2, &flag,
                                    &pflag, overlap_.data(), out, n_out, 1, 1),
              dsp_.context().raw());
        return n_out;
    }
    const std::vector<float> &overlap() const { return overlap_; }

private:
    Dsp &dsp_;
    std::vector<float> overlap_;
};

}  // namespace vorbis

namespace flac {

// lpc_predict::<N>(order, coeffs, coeff_shift, buf) via the dispatch of decode_linear (decoder.rs:487-504, 716-752):
// coeffs in bitstream order (the first multiplies the most recent sample); buf = warm-up samples then residuals.
inline void lpc_predict(Context &ctx, std::size_t order, const std::int32_t *coeffs, std::uint32_t coeff_shift, std::int32_t *buf,
                        std::size_t len) {
    if (order < 1 || order > 32 || order > len) throw std::invalid_argument("lpc_predict: order (decoder.rs:456-461)");
    if (coeff_shift > 31) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "lpc_predict: shift");
    std::int32_t c[32] = {0};
    for (std::size_t j = 0; j < order; ++j) c[j] = coeffs[j];
    const symaccel_flac_desc d{SYMACCEL_FLAC_LPC, (std::uint8_t)order, (std::uint8_t)coeff_shift, 0};
    check(symaccel_flac_restore(ctx.raw(), buf, &d, c, 1, len), ctx.raw());
}
// fixed_predict(order, buf) (decoder.rs:663-710)
inline void fixed_predict(Context &ctx, std::size_t order, std::int32_t *buf, std::size_t len) {
    if (order > 4) throw std::invalid_argument("fixed_predict: order > 4 (decoder.rs:664)");
    std::int32_t c[32] = {0};
    const symaccel_flac_desc d{SYMACCEL_FLAC_FIXED, (std::uint8_t)order, 0, 0};
    check(symaccel_flac_restore(ctx.raw(), buf, &d, c, 1, len), ctx.raw());
}
inline void restore_batch(Context &ctx, std::int32_t *buf, const symaccel_flac_desc *desc, const std::int32_t *coeffs,
                          std::size_t n_blocks, std::size_t blocksize) {
    check(symaccel_flac_restore(ctx.raw(), buf, desc, coeffs, n_blocks, blocksize), ctx.raw());
}
// A caller that owns a device batch plane (as the Batcher does for its FLAC / ALAC groups) gives its rows this pitch, in words: rows a power-of-two number of KiB
// apart -- 4096-sample blocks back to back -- alias on the HBM channels (symaccel_row_stride, include/symaccel.h; the reference has no counterpart: one Vec<i32>
// per channel, decoder.rs:199-242).  The device form over such a plane: the first `blocksize` words of a row are the subframe, the padding is left alone;
// d_pair_mode null = restore only, else restore + decorrelate + `<< out_shift` (decoder.rs:199-242 in one pass).
inline std::size_t row_stride(std::size_t blocksize) { return symaccel_row_stride(blocksize); }
inline void restore_strided_device(Context &ctx, std::int32_t *d_buf, const symaccel_flac_desc *d_desc, const std::int32_t *d_coeffs,
                                   const std::uint8_t *d_pair_mode, std::uint32_t out_shift, std::size_t n_blocks, std::size_t blocksize,
                                   std::size_t stride) {
    check(symaccel_flac_restore_strided_device(ctx.raw(), d_buf, d_desc, d_coeffs, d_pair_mode, out_shift, n_blocks, blocksize, stride), ctx.raw());
}
namespace detail {
inline void decorrelate(Context &ctx, std::uint8_t mode, std::int32_t *ch0, std::int32_t *ch1, std::size_t len) {
    check(symaccel_flac_decorrelate(ctx.raw(), &mode, ch0, ch1, 1, len, 0), ctx.raw());
}
}  // namespace detail
// decorrelate_left_side(left, side): side = left - side (decoder.rs:32-41)
inline void decorrelate_left_side(Context &ctx, const std::int32_t *left, std::int32_t *side, std::size_t len) {
    std::vector<std::int32_t> l(left, left + len);
    detail::decorrelate(ctx, 1, l.data(), side, len);
}
// decorrelate_mid_side(mid, side) in place (decoder.rs:43-70)
inline void decorrelate_mid_side(Context &ctx, std::int32_t *mid, std::int32_t *side, std::size_t len) {
    detail::decorrelate(ctx, 2, mid, side, len);
}
// decorrelate_right_side(right, side): side += right (decoder.rs:72-82)
inline void decorrelate_right_side(Context &ctx, const std::int32_t *right, std::int32_t *side, std::size_t len) {
    std::vector<std::int32_t> r(right, right + len);
    detail::decorrelate(ctx, 3, side, r.data(), len);
}

}  // namespace flac

namespace alac {

// ElementChannel (symphonia-codec-alac/src/lib.rs:71-80): the fields predict() reads.
struct ElementChannel {
    std::uint32_t bps = 16, mode = 0, shift = 0, lpc_order = 0;
    std::array<std::int32_t, 32> lpc_coeffs{};

    // predict(&mut self, out: &mut [i32]) -> Result<()> (lib.rs:165-264); decode_error on an invalid mode
    void predict(Context &ctx, std::int32_t *out, std::size_t len) const {
        if (mode > 0 && mode < 15) throw Error(Error::Kind::IoError, SYMACCEL_ERR_INVALID_ARG, "alac: invalid mode");
        if (lpc_order > 31 || bps == 0 || bps > 32) throw std::invalid_argument("alac::ElementChannel: field range");
        const symaccel_alac_desc d{(std::uint8_t)mode, (std::uint8_t)lpc_order, (std::uint8_t)shift, (std::uint8_t)bps};
        check(symaccel_alac_predict(ctx.raw(), out, &d, lpc_coeffs.data(), 1, len), ctx.raw());
    }
};
inline void predict_batch(Context &ctx, std::int32_t *buf, const symaccel_alac_desc *desc, const std::int32_t *coeffs,
                          std::size_t n_blocks, std::size_t blocksize) {
    check(symaccel_alac_predict(ctx.raw(), buf, desc, coeffs, n_blocks, blocksize), ctx.raw());
}
// predict over a device plane whose rows are `stride` words apart (flac::row_stride); d_pair_weight / d_pair_shift null = predict only, else with
// decorrelate_mid_side fused (lib.rs:541-560)
inline void predict_strided_device(Context &ctx, std::int32_t *d_buf, const symaccel_alac_desc *d_desc, const std::int32_t *d_coeffs,
                                   const std::int32_t *d_pair_weight, const std::uint8_t *d_pair_shift, std::size_t n_blocks,
                                   std::size_t blocksize, std::size_t stride) {
    check(symaccel_alac_predict_strided_device(ctx.raw(), d_buf, d_desc, d_coeffs, d_pair_weight, d_pair_shift, n_blocks, blocksize, stride), ctx.raw());
}
// decorrelate_mid_side(out0, out1, weight, shift) (lib.rs:664-671)
inline void decorrelate_mid_side(Context &ctx, std::int32_t *out0, std::int32_t *out1, std::size_t len, std::int32_t weight,
                                 std::uint8_t shift) {
    if (shift > 31) throw Error(Error::Kind::IoError, SYMACCEL_ERR_INVALID_ARG, "alac: mid_side_shift is greater than 31 bit");
    check(symaccel_alac_mid_side(ctx.raw(), &weight, &shift, out0, out1, 1, len), ctx.raw());
}

}  // namespace alac


// --------------------------------------------------------------------------------------------- codecs: the trait side
//
// symphonia_core::codecs::audio::AudioDecoder (symphonia-core/src/codecs/audio.rs:251-298):
//     fn reset(&mut self);  fn decode(&mut self, packet: &Packet) -> Result<GenericAudioBufferRef<'_>>;
//     fn finalize(&mut self) -> FinalizeResult;  fn last_decoded(&self) -> GenericAudioBufferRef<'_>;
// A GPU pays a launch and a PCIe round trip per call, so a drop-in decoder cannot transform one packet per decode():
// LookaheadDecoder keeps the trait's method set and its ownership rules (the decoder owns the buffer it returns a
// borrow of; the borrow is valid until the next &mut call; the buffer is cleared on error, audio.rs:278) and batches
// underneath: when decode(packet) finds nothing pre-computed for `packet`, it takes that packet plus up to K-1 packets
// the demuxer side can already see (the `peek` source: the shim wraps the FormatReader so that it reads ahead), runs ONE
// batch call over all of them -- every channel is a chain, the K packets are K consecutive frames of each chain, the
// state (delay lines, overlap, V FIFO) enters and leaves through the *_io buffers -- and hands the frames back one per
// call.  A packet that is not the one expected next (the caller seeked or dropped packets) invalidates the look-ahead.
// `Codec` supplies the packet type and the batch call (AacLc, Mp3 below); the entropy decode that produces the packets'
// spectra stays in the reference's CPU code.
namespace codecs {

template <class S>
struct AudioBufferRefT {  // GenericAudioBufferRef::F32 / ::S32 (audio/generic.rs:381-401): planar, one slice per channel
    std::vector<const S *> planes;
    std::size_t frames = 0;
    bool is_empty() const { return frames == 0; }
};
using AudioBufferRef = AudioBufferRefT<float>;          // the transform codecs
using AudioBufferRefS32 = AudioBufferRefT<std::int32_t>;  // FLAC (AudioBuffer<i32>, flac/decoder.rs:103)

// What last_decoded_bytes() of a decoder with an output format returns: the last packet as the bytes
// copy_bytes_to_vec_interleaved_as::<S> would give for the buffer decode() returns (audio/generic.rs:204-340), in the batcher's
// page-locked slot (valid, like every buffer of the trait, until the next &mut call).  Interleaved: `bytes` = frames * channels * sample
// bytes at `data`.  Planar (set_output(f, false)): channel c's frames * sample bytes at data + c * plane_stride.
struct DecodedBytes {
    const std::uint8_t *data = nullptr;
    std::size_t bytes = 0, frames = 0, channels = 0;
    SampleFormat format = SampleFormat::Native;
    std::size_t plane_stride = 0;  // bytes between the channels of a planar result; 0 = interleaved
};

struct FinalizeResult {  // codecs/audio.rs:230-236
    std::optional<bool> verify_ok;
};

// What LookaheadDecoder asks of a `Codec`.  Every codec derives from CodecBase and supplies the required members; the hooks have the
// defaults below, and a codec that needs one declares a member of the same name, which hides the default (LookaheadDecoder calls
// `codec_.x()` on the concrete type: no virtual call, no CRTP).
//
// Required of every codec:
//   Sample, Params, Packet; Codec(const Params &); channels();
//   decode_batch(ctx, batch, pcm)   one call of its own over the batch (a decoder without a Batcher, and the replay of one)
//   packet_frames(i), plane_offset(c, i, k)   where packet i of the last batch of k lies in channel c's plane
//   kBatchKind                      the SYMACCEL_BATCH_* kind of its submissions; 0 = it never goes through a Batcher
// ... and, with kBatchKind != 0:
//   batch_param(), batch_chains(k), batch_units(k)   the shape of a submission of k packets
//   take_state(slot)                the batch that was waited for is now the current one: carried state out of the slot, layout kept
//   fill_slot(batch, slot)          the parsed packets and the carried state into the page-locked slot -- for a codec whose layout depends
//                                   on the packets' content (AacLcCoded, Vorbis, Flac, Adpcm, Pcm).  One with fixed-size units sets
//   kDirect = true                  instead and supplies BatchView, view(slot, k), put(view, i, packet), extract(view, i), put_state(slot):
//                                   LookaheadDecoder fills the slot itself, and a parser may write straight into it (LookaheadDecoder::Direct)
// Everything else is a hook with a default:
struct CodecBase {
    template <class P>
    static std::uint64_t id(const P &p) { return p.ts; }  // what identifies a packet: Packet::ts
    void reset_state() {}       // AudioDecoder::reset: the carried state as after construction (default: nothing is carried)
    void attach(Batcher &) {}   // once, when the decoder is made on a batcher: what the codec registers with it or reads from it
    static constexpr bool kDirect = false;
    struct BatchView {};        // (kDirect: where every plane of a batch of k lies, in a slot or in the codec's own vectors)
    // set_output(): whether slot.out is the PCM the trait hands out as it comes back (false: take_state finishes it on the host)
    bool device_output_is_final() const { return true; }
    // A codec whose batcher kind delivers a format as [block][frame][channel] (ADPCM: the interleave group is one block's channels, the
    // blocks of a packet follow one another; PCM) says so: publish() then finds a packet's bytes at its first block, set_output() refuses
    // planar output, and `set_output_format(f)` tells the codec which of its two layouts plane_offset() is asked about
    static constexpr bool kBlockInterleave = false;
    void set_output_format(SampleFormat) {}
    // A codec whose slot shape depends on the packets of the batch (PCM: the frames of its longest packet) is shown the batch before the
    // slot is reserved: `prepare(batch)`
    template <class B>
    void prepare(const B &) {}
    // ... and one whose plane 0 may go up narrower says so per batch, before the slot is reserved: `input_format(batch)` = 0,
    // SYMACCEL_FMT_S16 or SYMACCEL_IN_FMT_ROWS (symaccel_batcher_reserve_io); its fill_slot() then writes plane 0 in that format.
    // narrow_batches() / wide_batches(): the batches it submitted as int16_t / int32_t; rows_sent(): the rows it sent with a width of their
    // own, at 2, 3 and 4 bytes a word; plane0_bytes(): the bytes of plane 0 it handed to the batcher in all
    template <class B>
    int input_format(const B &) { return 0; }
    std::size_t narrow_batches() const { return 0; }
    std::size_t wide_batches() const { return 0; }
    std::array<std::size_t, 3> rows_sent() const { return {0, 0, 0}; }
    std::size_t plane0_bytes() const { return 0; }
    // A codec with no host parse stage (ADPCM) finds a packet's own errors -- a rejected preamble, a packet shorter than its blocks -- when
    // the batch is assembled.  It keeps them per packet (`packet_error(i)`), the packet runs as silence, and decode() throws the error when
    // THAT packet's turn comes: a packet fails alone (codecs/audio.rs:273-278), its neighbours in the look-ahead batch keep their PCM.
    const Error *packet_error(std::size_t) const { return nullptr; }
    // A codec that verifies its stream (FLAC: the STREAMINFO MD5) says so with `kVerifies` -- LookaheadDecoder::set_verify then refuses a
    // change in mid-stream -- and is told about the decoder's life below it: `set_verify(bool)` (the registry's
    // AudioDecoderOptions::verify), `published(i)` when packet i of the current batch is handed out, `rewind()` when whatever was computed
    // beyond the last packet handed out is dropped (a seek, skipped packets, an error), `set_replaying(bool)` around the one-packet
    // replay, which must not count, and `finalize_result()`: its verdict over the packets handed out (default: none, like the reference's
    // decoders that verify nothing)
    static constexpr bool kVerifies = false;
    void set_verify(bool) {}
    void published(std::size_t) {}
    void rewind() {}
    void set_replaying(bool) {}
    FinalizeResult finalize_result() { return FinalizeResult{}; }

    // Carried state: one plane = its host copy and its index in slot.state.  `state_planes()` of a codec lists them; put_state / take_state
    // (and a fill_slot that writes its own) are store_state / load_state over that one list.
    struct StatePlane {
        void *host;
        std::size_t bytes;
        int index;
    };
    template <class T>
    static StatePlane plane_of(std::vector<T> &v, int index) { return StatePlane{v.data(), v.size() * sizeof(T), index}; }
    template <class Planes>
    static void store_state(const Planes &planes, const symaccel_batch_slot &slot) {
        for (const StatePlane &p : planes) std::memcpy(slot.state[p.index], p.host, p.bytes);
    }
    template <class Planes>
    static void load_state(const Planes &planes, const symaccel_batch_slot &slot) {
        for (const StatePlane &p : planes) std::memcpy(p.host, slot.state[p.index], p.bytes);
    }
};

// With a `Batcher` (second constructor) the same decoder coalesces ACROSS streams: its batches are submitted to the process-wide
// batcher instead of being transformed by a call of their own, and the next batch is submitted early -- as soon as half of the
// current one has been handed out -- so that by the time this stream needs it, the decoders of the other streams have submitted
// theirs and one launch (one PCIe round trip) serves all of them.  The returned planes then point into the batcher's page-locked
// result slot (valid, like every buffer of the trait, until the next &mut call).
template <class Codec>
class LookaheadDecoder {
public:
    using Packet = typename Codec::Packet;
    using Sample = typename Codec::Sample;                // f32 for the transform codecs, i32 for FLAC
    using Buffer = AudioBufferRefT<Sample>;
    using Peek = std::function<std::optional<Packet>()>;  // the next packet of the same track the demuxer can see, if any

    LookaheadDecoder(Context &ctx, const typename Codec::Params &params, std::size_t lookahead, Peek peek)
        : ctx_(ctx), codec_(params), lookahead_(lookahead < 1 ? 1 : lookahead), peek_(std::move(peek)) {
        reset();
    }
    LookaheadDecoder(Batcher &batcher, const typename Codec::Params &params, std::size_t lookahead, Peek peek)
        : ctx_(batcher.context()), codec_(params), lookahead_(lookahead < 1 ? 1 : lookahead), peek_(std::move(peek)),
          batcher_(Codec::kBatchKind ? &batcher : nullptr) {
        if (batcher_) codec_.attach(batcher);  // (what a codec registers with the batcher once: AacLcCoded's band tables)
        reset();
    }
    // Zero-copy parse: a front end that can parse the demuxer's next packet STRAIGHT INTO the batcher's page-locked slot.  The batch
    // length is fixed first -- `avail()` = the packets of this track the demuxer can see now --, the slot is reserved for it, and
    // `parse_into(view, i)` parses the next packet into position i of the batch (`view`: the codec's BatchView, the destination of
    // every plane in the chain-major layout) and returns its id; nullopt = no packet after all (the batch is re-packed shorter).
    // Nothing is copied between the parser's output and the DMA source.  For codecs with `kDirect` (fixed-size units: AacLc, Mp3,
    // Mp3Huffman); the Rust twin: `BatchCodec::reserve` / `commit` (bindings/rust/symphonia-accel-hip/src/lookahead.rs).
    struct Direct {
        std::function<std::size_t()> avail;
        std::function<std::optional<std::uint64_t>(const typename Codec::BatchView &, std::size_t)> parse_into;
    };
    LookaheadDecoder(Batcher &batcher, const typename Codec::Params &params, std::size_t lookahead, Direct direct)
        : ctx_(batcher.context()), codec_(params), lookahead_(lookahead < 1 ? 1 : lookahead), batcher_(&batcher), direct_(std::move(direct)) {
        static_assert(Codec::kDirect, "this codec's batch layout depends on the packets' content: use the Peek form");
        if (!direct_.avail || !direct_.parse_into) throw std::invalid_argument("LookaheadDecoder: direct source");
        codec_.attach(batcher);
        reset();
    }
    ~LookaheadDecoder() { drop_tickets(); }
    LookaheadDecoder(const LookaheadDecoder &) = delete;
    LookaheadDecoder &operator=(const LookaheadDecoder &) = delete;

    // AudioDecoder::reset (audio.rs:252-257): "must be called after a seek"; state as after construction
    void reset() {
        drop_tickets();
        codec_.reset_state();
        ready_.clear();
        head_ = 0;
        have_last_packet_ = false;
        clear_last();
    }

    // AudioDecoder::decode (audio.rs:259-281)
    const Buffer &decode(const Packet &packet) {
        if (head_ < ready_.size() && ready_[head_] != Codec::id(packet)) {
            // Not the packet the look-ahead was computed for: the caller skipped packets without reset().  A
            // frame-by-frame decoder would now continue from the state the LAST RETURNED packet left, but the carried
            // state here is already that of the end of the batch.  Every codec on this path has a one-packet memory
            // (the delay line / overlap / V FIFO after a packet depend on that packet's input alone -- the same property
            // the kernels' segment halo uses), so replaying the last returned packet rebuilds exactly that state.
            drop_lookahead();
            if (have_last_packet_) replay_last();
        }
        if (head_ >= ready_.size()) {
            try {
                if (next_live_ && !next_ids_.empty() && next_ids_[0] == Codec::id(packet)) {
                    take_next();  // the batch submitted ahead starts with this packet
                } else {
                    // (a batch submitted ahead for packets the caller then skipped is dropped unseen: the carried state is still
                    // the one the last returned packet left, because the current batch was handed out to its end)
                    if (next_live_) drop_lookahead();
                    fill(packet);
                }
            } catch (...) {
                clear_last();  // audio.rs:278: "implementors of this function must clear the internal buffer if an error occurs"
                drop_tickets();
                ready_.clear();
                head_ = 0;
                throw;
            }
        }
        if (const Error *e = codec_.packet_error(head_)) {
            const Error own = *e;
            ++head_;       // the packet is consumed: the rest of the batch stays
            clear_last();  // audio.rs:278
            throw own;
        }
        publish(head_++);
        last_packet_ = packet;
        have_last_packet_ = true;
        if (batcher_) {
            // half of the batch handed out: the next one is submitted (the other streams' decoders do the same around now); a
            // quarter left: whatever is pending goes to the device, so that the copies and the kernels run while the rest is consumed
            const std::size_t left = ready_.size() - head_;
            if (!next_live_ && 2 * left <= ready_.size()) submit_ahead();
            if (next_live_ && !hinted_ && 4 * left <= ready_.size()) {
                hinted_ = true;
                batcher_->hint();
            }
        }
        return last_;
    }

    // AudioDecoder::finalize (audio.rs:283-290): the codec's verdict over the packets handed out so far (the f32 codecs verify
    // nothing, like the reference's)
    FinalizeResult finalize() { return codec_.finalize_result(); }
    // AudioDecoderOptions::verify for a codec that can (before the first decode()); the others behave as ever
    void set_verify(bool on) {
        if (Codec::kVerifies && (cur_live_ || next_live_ || head_ < ready_.size())) throw std::logic_error("LookaheadDecoder::set_verify: before the first decode()");
        codec_.set_verify(on);
    }
    const Buffer &last_decoded() const { return last_; }
    // Deliver the PCM in the caller's sample format, converted (and interleaved) in the batcher's scatter: what crosses the link is the
    // bytes the caller wants (symaccel_batcher_reserve_fmt).  decode() then keeps returning the frame count, the planar ref holds no
    // planes, and last_decoded_bytes() is the packet.  For decoders on a Batcher; between batches only: before the first decode() or
    // right after reset().  SampleFormat::Native restores the planes.  (A FLAC stream that is not two channels wide is left-justified
    // on the host, after the scatter: Error{Unsupported}.)
    void set_output(SampleFormat format, bool interleaved = true) {
        if (format != SampleFormat::Native) {
            if (!batcher_ || Codec::kBatchKind == 0) throw std::invalid_argument("LookaheadDecoder::set_output: the conversion happens in the batcher's scatter");
            if (sample_bytes(format) == 0 || codec_.channels() > 8) throw std::invalid_argument("LookaheadDecoder::set_output: format / channels");
            if (!codec_.device_output_is_final()) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "set_output: this stream's planes are finished on the host");
            if (Codec::kBlockInterleave && !interleaved) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "set_output: this codec's kernel writes interleaved frames");
        }
        if (cur_live_ || next_live_ || head_ < ready_.size()) throw std::logic_error("LookaheadDecoder::set_output: between batches only (before decode() or after reset())");
        codec_.set_output_format(format);
        out_fmt_ = format;
        out_interleaved_ = interleaved;
        clear_last();
    }
    const DecodedBytes &last_decoded_bytes() const { return bytes_; }
    std::size_t lookahead() const { return lookahead_; }
    std::size_t batches_run() const { return batches_; }
    // the batches this decoder submitted with plane 0 as int16_t / as int32_t (a codec with input_format(): Flac; 0 for the others)
    std::size_t narrow_batches() const { return codec_.narrow_batches(); }
    std::size_t wide_batches() const { return codec_.wide_batches(); }
    // ... the rows it sent with a width of their own (Batcher::InputMode::Rows) at 2, 3 and 4 bytes a word, and the bytes of plane 0 in all
    std::array<std::size_t, 3> rows_sent() const { return codec_.rows_sent(); }
    std::size_t plane0_bytes() const { return codec_.plane0_bytes(); }

private:
    std::vector<Packet> gather(const Packet *first) {
        std::vector<Packet> batch;
        if (first) batch.push_back(*first);
        // packets pulled earlier whose frames were dropped by a discontinuity are not replayed: the demuxer moved on
        while (batch.size() < lookahead_) {
            std::optional<Packet> nxt = peek_ ? peek_() : std::nullopt;
            if (!nxt) break;
            batch.push_back(std::move(*nxt));
        }
        return batch;
    }
    void fill(const Packet &first) {
        if (direct_.avail) {
            if constexpr (Codec::kDirect) {
                submit_direct(&first);
                take_next();
                return;
            }
        }
        std::vector<Packet> batch = gather(&first);
        if (batcher_) {
            if constexpr (Codec::kBatchKind != 0) {
                submit(batch);
                take_next();
                return;
            }
        }
        codec_.decode_batch(ctx_, batch, pcm_);
        pcm_base_ = pcm_.data();
        ++batches_;
        ready_.clear();
        for (const Packet &p : batch) ready_.push_back(Codec::id(p));
        batch_len_ = batch.size();
        head_ = 0;
    }
    // ---- batcher mode
    void submit(const std::vector<Packet> &batch) {
        if constexpr (Codec::kBatchKind != 0) {
            symaccel_batch_slot slot;
            codec_.prepare(batch);
            reserve(batch.size(), &slot, &next_ticket_, codec_.input_format(batch));
            next_live_ = true;
            try {  // the parsed packets and the carried state go into the page-locked slot
                if constexpr (Codec::kDirect) {
                    const typename Codec::BatchView view = codec_.view(slot, batch.size());
                    for (std::size_t i = 0; i < batch.size(); ++i) codec_.put(view, i, batch[i]);
                    codec_.put_state(slot);
                } else {
                    codec_.fill_slot(batch, slot);
                }
            } catch (...) {
                symaccel_batcher_release(batcher_->raw(), next_ticket_);
                next_live_ = false;
                throw;
            }
            check(symaccel_batcher_commit(batcher_->raw(), next_ticket_), ctx_.raw());
            next_ids_.clear();
            for (const Packet &p : batch) next_ids_.push_back(Codec::id(p));
            hinted_ = false;
        }
    }
    // a slot for a batch of n packets: the native planes (SampleFormat::Native is out_fmt 0: the channel count is then not read), or
    // (set_output) the interleave groups of the caller's format; in_fmt: plane 0 as int16_t, widened in the gather (input_format())
    void reserve(std::size_t n, symaccel_batch_slot *sl, std::uint64_t *t, int in_fmt = 0) {
        if constexpr (Codec::kBatchKind != 0)
            batcher_->reserve_io(Codec::kBatchKind, codec_.batch_param(), codec_.batch_chains(n), codec_.batch_units(n), in_fmt, static_cast<int>(out_fmt_),
                                 out_interleaved_ ? (int)codec_.channels() : 1, sl, t);
    }
    void replay_last() {
        std::vector<Packet> one(1, last_packet_);
        struct Replaying {  // (a verifying codec counts this packet once: when it was handed out)
            Codec &c;
            explicit Replaying(Codec &codec) : c(codec) { c.set_replaying(true); }
            ~Replaying() { c.set_replaying(false); }
        } replaying(codec_);
        if (batcher_) {
            if constexpr (Codec::kBatchKind != 0) {  // (through the batcher: the context is not ours to call while a batcher drives it)
                submit(one);
                symaccel_batch_slot slot;
                const int st = symaccel_batcher_wait(batcher_->raw(), next_ticket_, &slot);
                if (st == SYMACCEL_OK) codec_.take_state(slot);
                symaccel_batcher_release(batcher_->raw(), next_ticket_);
                next_live_ = false;
                next_ids_.clear();
                check(st, ctx_.raw());
                return;
            }
        }
        std::vector<Sample> scratch;
        codec_.decode_batch(ctx_, one, scratch);
    }
    void submit_ahead() {
        // the state the next batch starts from is the one the current batch left: known since take_next() copied it out
        if (direct_.avail) {
            if constexpr (Codec::kDirect) {
                submit_direct(nullptr);
                return;
            }
        }
        std::vector<Packet> batch = gather(nullptr);
        if (!batch.empty()) submit(batch);
    }
    // the direct form of submit(): reserve for the packets the demuxer can see, parse them into the slot, commit
    void submit_direct(const Packet *first) {
        if constexpr (Codec::kDirect) {
            const std::size_t head = first ? 1 : 0;
            std::size_t k = head + std::min(lookahead_ - head, direct_.avail());
            if (k == 0) return;
            symaccel_batch_slot slot;
            reserve(k, &slot, &next_ticket_);
            next_live_ = true;
            next_ids_.clear();
            try {
                typename Codec::BatchView view = codec_.view(slot, k);
                std::size_t j = 0;
                if (first) {
                    codec_.put(view, 0, *first);
                    next_ids_.push_back(Codec::id(*first));
                    j = 1;
                }
                for (; j < k; ++j) {
                    const std::optional<std::uint64_t> id = direct_.parse_into(view, j);
                    if (!id) break;
                    next_ids_.push_back(*id);
                }
                if (j == 0) {  // nothing there after all
                    symaccel_batcher_release(batcher_->raw(), next_ticket_);
                    next_live_ = false;
                    return;
                }
                if (j < k) {
                    // fewer packets than the demuxer announced (a corrupt one ends the batch): the rows move to a slot of the right
                    // shape -- units are part of the layout AND of the state the batch leaves -- and the long one goes back unused
                    symaccel_batch_slot shorter;
                    std::uint64_t t2 = 0;
                    reserve(j, &shorter, &t2);
                    typename Codec::BatchView to = codec_.view(shorter, j);
                    for (std::size_t i = 0; i < j; ++i) codec_.put(to, i, codec_.extract(view, i));
                    symaccel_batcher_release(batcher_->raw(), next_ticket_);
                    next_ticket_ = t2;
                    slot = shorter;
                }
                codec_.put_state(slot);
            } catch (...) {
                symaccel_batcher_release(batcher_->raw(), next_ticket_);
                next_live_ = false;
                throw;
            }
            check(symaccel_batcher_commit(batcher_->raw(), next_ticket_), ctx_.raw());
            hinted_ = false;
        }
    }
    void take_next() {
        if constexpr (Codec::kBatchKind != 0) {
            symaccel_batch_slot slot;
            const int st = symaccel_batcher_wait(batcher_->raw(), next_ticket_, &slot);
            if (st != SYMACCEL_OK) {
                symaccel_batcher_release(batcher_->raw(), next_ticket_);
                next_live_ = false;
                check(st, ctx_.raw());
            }
            if (cur_live_) symaccel_batcher_release(batcher_->raw(), cur_ticket_);
            cur_ticket_ = next_ticket_;
            cur_live_ = true;
            next_live_ = false;
            codec_.take_state(slot);
            pcm_base_ = out_fmt_ == SampleFormat::Native ? static_cast<const Sample *>(slot.out) : nullptr;
            out_base_ = static_cast<const std::uint8_t *>(slot.out);
            out_valid_ = slot.out_bytes;
            ready_.swap(next_ids_);
            next_ids_.clear();
            batch_len_ = ready_.size();
            head_ = 0;
            ++batches_;
        }
    }
    void drop_tickets() {
        codec_.rewind();
        if (!batcher_) return;
        if (next_live_) {
            symaccel_batcher_wait(batcher_->raw(), next_ticket_, nullptr);  // (its result is not wanted, its slot must be idle)
            symaccel_batcher_release(batcher_->raw(), next_ticket_);
            next_live_ = false;
        }
        if (cur_live_) {
            symaccel_batcher_release(batcher_->raw(), cur_ticket_);
            cur_live_ = false;
        }
        next_ids_.clear();
        pcm_base_ = nullptr;
    }
    void drop_lookahead() {
        drop_tickets();
        clear_last();
        ready_.clear();
        head_ = 0;
    }
    void publish(std::size_t i) {
        codec_.published(i);
        // where packet i of the last batch lies in a channel's plane is the codec's business: fixed-size frames are
        // [channel][packet][frames]; Vorbis packs (prev_n + n) / 4 samples per packet and none for the first one
        const std::size_t nch = codec_.channels();
        last_.frames = codec_.packet_frames(i);
        if (out_fmt_ != SampleFormat::Native) {
            if constexpr (Codec::kBatchKind != 0) {
                // The converted slot holds the interleave groups back to back, each `per_chain` samples of every chain of it (the native
                // plane's length; for Vorbis what the flags account for).  A packet is the frame range plane_offset() names in the
                // native layout: chain = offset / native plane length, frames into the chain = the remainder.
                last_.planes.assign(nch, nullptr);
                const std::size_t sb = sample_bytes(out_fmt_), n_chains = codec_.batch_chains(batch_len_);
                std::size_t native = 0;
                check(symaccel_batcher_plane_bytes(Codec::kBatchKind, codec_.batch_param(), codec_.batch_units(batch_len_), nullptr, nullptr, &native), ctx_.raw());
                native /= 4;
                const std::size_t per_chain = out_valid_ / (n_chains * sb), at0 = codec_.plane_offset(0, i, batch_len_);
                bytes_.frames = last_.frames;
                bytes_.channels = nch;
                bytes_.format = out_fmt_;
                if constexpr (Codec::kBlockInterleave) {
                    bytes_.data = out_base_ + at0 * sb;  // (plane_offset(0, i) = the samples in front of the packet's first block, all channels)
                    bytes_.bytes = last_.frames * nch * sb;
                    bytes_.plane_stride = 0;
                } else if (out_interleaved_) {
                    bytes_.data = out_base_ + ((at0 / native / nch) * per_chain + at0 % native) * nch * sb;
                    bytes_.bytes = last_.frames * nch * sb;
                    bytes_.plane_stride = 0;
                } else {
                    const std::size_t at1 = nch > 1 ? codec_.plane_offset(1, i, batch_len_) : at0;
                    bytes_.data = out_base_ + ((at0 / native) * per_chain + at0 % native) * sb;
                    bytes_.bytes = last_.frames * sb;
                    bytes_.plane_stride = ((at1 / native) - (at0 / native)) * per_chain * sb;
                }
            }
            return;
        }
        last_.planes.resize(nch);
        for (std::size_t c = 0; c < nch; ++c) last_.planes[c] = pcm_base_ + codec_.plane_offset(c, i, batch_len_);
    }
    void clear_last() {
        last_.planes.assign(codec_.channels(), nullptr);
        last_.frames = 0;
        bytes_ = DecodedBytes{};
    }

    Context &ctx_;
    Codec codec_;
    std::size_t lookahead_;
    Peek peek_;
    Batcher *batcher_ = nullptr;
    Direct direct_{};                        // (empty: the Peek form)
    std::vector<Sample> pcm_;                // [channel][packet of the batch][frames_per_packet]: planar per packet
    const Sample *pcm_base_ = nullptr;       // pcm_.data(), or the batcher's result slot of the current batch
    SampleFormat out_fmt_ = SampleFormat::Native;  // set_output
    bool out_interleaved_ = true;
    const std::uint8_t *out_base_ = nullptr;  // the result slot as bytes, out_valid_ of them valid
    std::size_t out_valid_ = 0;
    DecodedBytes bytes_;
    std::vector<std::uint64_t> ready_;       // ids of the batch's packets, in order
    std::vector<std::uint64_t> next_ids_;    // ... of the batch submitted ahead
    std::uint64_t cur_ticket_ = 0, next_ticket_ = 0;
    bool cur_live_ = false, next_live_ = false, hinted_ = false;
    Packet last_packet_{};                   // the packet decode() returned last (replayed after a discontinuity)
    bool have_last_packet_ = false;
    std::size_t head_ = 0, batch_len_ = 0, batches_ = 0;
    Buffer last_;
};

// AAC-LC: one packet = one raw_data_block = 1024 frames per channel.  What the CPU side (reference parser + spectral
// tools) hands over per channel: the dequantised coefficients Ics::synth_channel would give Dsp::synth, the window
// sequence and the window shapes (ics/mod.rs:449-468).
struct AacLc : CodecBase {
    using Sample = float;
    struct Params {
        std::size_t channels = 2;
    };
    struct Packet {
        std::uint64_t ts = 0;                // Packet::ts: identifies the packet
        std::vector<float> coeffs;           // [channel][1024]
        std::vector<std::uint8_t> side;      // [channel]: SYMACCEL_AAC_SIDE(seq, shape, prev_shape)
    };
    explicit AacLc(const Params &p) : nch_(p.channels), delay_(p.channels * 1024, 0.0f) {}
    std::size_t channels() const { return nch_; }
    std::size_t packet_frames(std::size_t) const { return 1024; }
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t k) const { return (c * k + i) * 1024; }
    void reset_state() { std::fill(delay_.begin(), delay_.end(), 0.0f); }  // AacDecoder::reset: delay lines zeroed
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<float> &pcm) {
        const std::size_t k = batch.size();
        in_.resize(nch_ * k * 1024);
        side_.resize(nch_ * k);
        pcm.resize(nch_ * k * 1024);
        const BatchView v{in_.data(), side_.data(), k, nch_};
        for (std::size_t i = 0; i < k; ++i) put(v, i, batch[i]);
        check(symaccel_aac_synth(ctx.raw(), in_.data(), side_.data(), delay_.data(), pcm.data(), nch_, k), ctx.raw());
    }
    // the cross-stream batcher's view of the same batch (LookaheadDecoder's second constructor)
    static constexpr int kBatchKind = SYMACCEL_BATCH_AAC_SYNTH;
    static constexpr bool kDirect = true;
    int batch_param() const { return 0; }
    std::size_t batch_chains(std::size_t) const { return nch_; }  // a submission of k packets: nch chains of k units
    std::size_t batch_units(std::size_t k) const { return k; }
    // where packet i of a batch of k lies in a slot's planes (what a parser that writes straight into the slot needs: LookaheadDecoder::Direct)
    struct BatchView {
        float *coeffs = nullptr;
        std::uint8_t *side = nullptr;
        std::size_t k = 0, nch = 0;
        float *coeffs_at(std::size_t c, std::size_t i) const { return coeffs + (c * k + i) * 1024; }
        std::uint8_t &side_at(std::size_t c, std::size_t i) const { return side[c * k + i]; }
    };
    BatchView view(const symaccel_batch_slot &slot, std::size_t k) const {
        return BatchView{static_cast<float *>(slot.input[0]), static_cast<std::uint8_t *>(slot.input[1]), k, nch_};
    }
    static void put(const BatchView &v, std::size_t i, const Packet &p) {  // (the one placement: a slot's planes or decode_batch's own)
        if (p.coeffs.size() != v.nch * 1024 || p.side.size() != v.nch) throw std::invalid_argument("AacLc: packet shape");
        for (std::size_t c = 0; c < v.nch; ++c) {
            std::copy_n(p.coeffs.data() + c * 1024, 1024, v.coeffs_at(c, i));
            v.side_at(c, i) = p.side[c];
        }
    }
    Packet extract(const BatchView &v, std::size_t i) const {
        Packet p;
        p.coeffs.resize(nch_ * 1024);
        p.side.resize(nch_);
        for (std::size_t c = 0; c < nch_; ++c) {
            std::copy_n(v.coeffs_at(c, i), 1024, p.coeffs.data() + c * 1024);
            p.side[c] = v.side_at(c, i);
        }
        return p;
    }
    std::array<StatePlane, 1> state_planes() { return {{plane_of(delay_, 0)}}; }
    void put_state(const symaccel_batch_slot &slot) { store_state(state_planes(), slot); }
    void take_state(const symaccel_batch_slot &slot) { load_state(state_planes(), slot); }

private:
    std::size_t nch_;
    std::vector<float> delay_, in_;
    std::vector<std::uint8_t> side_;
};

// AAC-LC one stage earlier: what the spectrum decoder produces (cpe.rs:110-157 and ics/mod.rs:449-468 still to come) -- the
// coefficients as decoded (mid / side or intensity coded where the descriptors say so), per jointly coded channel pair its
// descriptor, and the TNS filters of the packet; joint stereo, TNS and Dsp::synth run on the device (symaccel_aac_decode_pipelined,
// or SYMACCEL_BATCH_AAC_DECODE through the batcher: the pair frames with TNS take a list pass, the filters run, one walk synthesises).
struct AacLcCoded : CodecBase {
    using Sample = float;
    struct Params {
        std::size_t channels = 2;
        std::vector<std::uint16_t> swb_long, swb_short;  // the stream's scale-factor-band offsets (n + 1 values each)
    };
    struct Packet {
        std::uint64_t ts = 0;
        std::vector<float> coeffs;                                       // [channel][1024]
        std::vector<std::uint8_t> side;                                  // [channel]
        std::vector<std::pair<std::size_t, symaccel_aac_js_frame>> joint;  // (left channel of the pair, its descriptor)
        std::vector<symaccel_aac_tns_filter> tns;                        // frame = channel
    };
    explicit AacLcCoded(const Params &p) : nch_(p.channels), swb_long_(p.swb_long), swb_short_(p.swb_short), delay_(p.channels * 1024, 0.0f) {
        if (swb_long_.size() < 2 || swb_short_.size() < 2) throw std::invalid_argument("AacLcCoded: band tables");
    }
    std::size_t channels() const { return nch_; }
    std::size_t packet_frames(std::size_t) const { return 1024; }
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t k) const { return (c * k + i) * 1024; }
    void reset_state() { std::fill(delay_.begin(), delay_.end(), 0.0f); }
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<float> &pcm) {
        const std::size_t k = batch.size();
        in_.resize(nch_ * k * 1024);
        side_.resize(nch_ * k);
        pcm.resize(nch_ * k * 1024);
        describe(batch, in_.data(), side_.data());
        const std::size_t n_pairs = pairs_.size() / 2;
        check(symaccel_aac_decode_pipelined(ctx.raw(), in_.data(), side_.data(), n_pairs ? pairs_.data() : nullptr, n_pairs ? js_.data() : nullptr,
                                            n_pairs, swb_long_.data(), (int)swb_long_.size() - 1, swb_short_.data(), (int)swb_short_.size() - 1,
                                            tns_.empty() ? nullptr : tns_.data(), tns_.size(), delay_.data(), pcm.data(), nch_, k, 0),
              ctx.raw());
    }
    static constexpr int kBatchKind = SYMACCEL_BATCH_AAC_DECODE;  // (not kDirect: the descriptor blob is assembled from the whole batch)
    void attach(Batcher &b) {
        check(symaccel_batcher_aac_bands(b.raw(), swb_long_.data(), (int)swb_long_.size() - 1, swb_short_.data(), (int)swb_short_.size() - 1, &bands_),
              b.context().raw());
    }
    int batch_param() const { return bands_; }
    std::size_t batch_chains(std::size_t) const { return nch_; }  // a submission of k packets: nch chains of k units
    std::size_t batch_units(std::size_t k) const { return k; }
    void fill_slot(const std::vector<Packet> &batch, const symaccel_batch_slot &slot) {
        const std::size_t k = batch.size();
        describe(batch, static_cast<float *>(slot.input[0]), static_cast<std::uint8_t *>(slot.input[1]));
        // the descriptor blob (include/symaccel.h, SYMACCEL_BATCH_AAC_DECODE): header, pair list, js rows, filters, 16-byte aligned parts
        const std::size_t n_pairs = pairs_.size() / 2;
        const std::size_t off_js = 16 + ((n_pairs * 8 + 15) & ~(std::size_t)15);
        const std::size_t off_tns = off_js + ((n_pairs * k * sizeof(symaccel_aac_js_frame) + 15) & ~(std::size_t)15);
        if (off_tns + tns_.size() * sizeof(symaccel_aac_tns_filter) > slot.input_bytes[2]) throw std::invalid_argument("AacLcCoded: more than 8 TNS filters per channel-frame");
        char *blob = static_cast<char *>(slot.input[2]);
        const std::uint32_t header[4] = {(std::uint32_t)n_pairs, (std::uint32_t)tns_.size(), 0u, 0u};
        std::memcpy(blob, header, 16);
        if (n_pairs) {
            std::memcpy(blob + 16, pairs_.data(), n_pairs * 8);
            std::memcpy(blob + off_js, js_.data(), n_pairs * k * sizeof(symaccel_aac_js_frame));
        }
        if (!tns_.empty()) std::memcpy(blob + off_tns, tns_.data(), tns_.size() * sizeof(symaccel_aac_tns_filter));
        store_state(state_planes(), slot);
    }
    std::array<StatePlane, 1> state_planes() { return {{plane_of(delay_, 0)}}; }
    void take_state(const symaccel_batch_slot &slot) { load_state(state_planes(), slot); }

private:
    // the batch in the entry points' terms: chain-major spectra + side bytes, the pairs coded jointly anywhere in the batch, their
    // descriptors [pair][packet] (a packet in which a pair is not jointly coded gets the empty descriptor), the filters re-based
    void describe(const std::vector<Packet> &batch, float *in, std::uint8_t *side) {
        const std::size_t k = batch.size();
        std::vector<std::size_t> lefts;
        for (std::size_t i = 0; i < k; ++i) {
            const Packet &p = batch[i];
            if (p.coeffs.size() != nch_ * 1024 || p.side.size() != nch_) throw std::invalid_argument("AacLcCoded: packet shape");
            for (std::size_t c = 0; c < nch_; ++c) {
                std::copy_n(p.coeffs.data() + c * 1024, 1024, in + (c * k + i) * 1024);
                side[c * k + i] = p.side[c];
            }
            for (const auto &j : p.joint)
                if (j.first + 1 < nch_ && std::find(lefts.begin(), lefts.end(), j.first) == lefts.end()) lefts.push_back(j.first);
        }
        std::sort(lefts.begin(), lefts.end());
        pairs_.clear();
        for (std::size_t l : lefts) {
            pairs_.push_back((std::int32_t)l);
            pairs_.push_back((std::int32_t)l + 1);
        }
        symaccel_aac_js_frame none{};
        none.num_windows = 1;
        js_.assign(lefts.size() * k, none);
        tns_.clear();
        for (std::size_t i = 0; i < k; ++i) {
            for (const auto &j : batch[i].joint) {
                const auto it = std::find(lefts.begin(), lefts.end(), j.first);
                if (it != lefts.end()) js_[(std::size_t)(it - lefts.begin()) * k + i] = j.second;
            }
            for (symaccel_aac_tns_filter f : batch[i].tns) {
                f.frame = (std::uint32_t)((std::size_t)f.frame * k + i);  // [channel][packet of the batch]
                tns_.push_back(f);
            }
        }
    }
    std::size_t nch_;
    std::vector<std::uint16_t> swb_long_, swb_short_;
    std::vector<float> delay_, in_;
    std::vector<std::uint8_t> side_;
    std::vector<std::int32_t> pairs_;
    std::vector<symaccel_aac_js_frame> js_;
    std::vector<symaccel_aac_tns_filter> tns_;
    int bands_ = -1;
};

// MPEG-1/2 Layer III: one packet = one frame = `granules` granules of 576 frames per channel (2 for MPEG-1, 1 for
// MPEG-2 / 2.5, common.rs:173-178).  Per granule-channel: the requantised, stereo-processed samples and the side fields
// the synthesis tail reads (layer3/mod.rs:440-476).
struct Mp3 : CodecBase {
    using Sample = float;
    struct Params {
        std::size_t channels = 2;
        std::size_t granules = 2;
        int sample_rate_idx = 0;
    };
    struct Packet {
        std::uint64_t ts = 0;
        std::vector<float> xr;                 // [granule][channel][576]
        std::vector<symaccel_mp3_side> side;   // [granule][channel]
    };
    explicit Mp3(const Params &p)
        : nch_(p.channels), ngr_(p.granules), sr_(p.sample_rate_idx), overlap_(p.channels * 576, 0.0f), vvec_(p.channels * 1024, 0.0f),
          vfront_(p.channels, 0) {}
    std::size_t channels() const { return nch_; }
    std::size_t packet_frames(std::size_t) const { return 576 * ngr_; }
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t k) const { return (c * k + i) * 576 * ngr_; }
    void reset_state() {  // MpaDecoder::reset: fresh State (overlap and SynthesisState::default())
        std::fill(overlap_.begin(), overlap_.end(), 0.0f);
        std::fill(vvec_.begin(), vvec_.end(), 0.0f);
        std::fill(vfront_.begin(), vfront_.end(), 0);
    }
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<float> &pcm) {
        const std::size_t k = batch.size(), g = k * ngr_;
        in_.resize(nch_ * g * 576);
        side_.resize(nch_ * g);
        pcm.resize(nch_ * g * 576);
        const BatchView v{in_.data(), side_.data(), k, nch_, ngr_};
        for (std::size_t i = 0; i < k; ++i) put(v, i, batch[i]);
        check(symaccel_mp3_synth(ctx.raw(), in_.data(), side_.data(), sr_, overlap_.data(), vvec_.data(), vfront_.data(), pcm.data(), nch_, g),
              ctx.raw());
    }
    static constexpr int kBatchKind = SYMACCEL_BATCH_MP3_SYNTH;
    static constexpr bool kDirect = true;
    int batch_param() const { return sr_; }
    std::size_t batch_chains(std::size_t) const { return nch_; }
    std::size_t batch_units(std::size_t k) const { return k * ngr_; }
    struct BatchView {  // granule gr of packet i of channel c is unit i * ngr + gr of chain c
        float *xr = nullptr;
        symaccel_mp3_side *side = nullptr;
        std::size_t k = 0, nch = 0, ngr = 0;
        std::size_t unit(std::size_t c, std::size_t i, std::size_t gr) const { return c * k * ngr + i * ngr + gr; }
    };
    BatchView view(const symaccel_batch_slot &slot, std::size_t k) const {
        return BatchView{static_cast<float *>(slot.input[0]), static_cast<symaccel_mp3_side *>(slot.input[1]), k, nch_, ngr_};
    }
    static void put(const BatchView &v, std::size_t i, const Packet &p) {
        if (p.xr.size() != v.ngr * v.nch * 576 || p.side.size() != v.ngr * v.nch) throw std::invalid_argument("Mp3: packet shape");
        for (std::size_t gr = 0; gr < v.ngr; ++gr)
            for (std::size_t c = 0; c < v.nch; ++c) {
                std::copy_n(p.xr.data() + (gr * v.nch + c) * 576, 576, v.xr + v.unit(c, i, gr) * 576);
                v.side[v.unit(c, i, gr)] = p.side[gr * v.nch + c];
            }
    }
    Packet extract(const BatchView &v, std::size_t i) const {
        Packet p;
        p.xr.resize(ngr_ * nch_ * 576);
        p.side.resize(ngr_ * nch_);
        for (std::size_t gr = 0; gr < ngr_; ++gr)
            for (std::size_t c = 0; c < nch_; ++c) {
                std::copy_n(v.xr + v.unit(c, i, gr) * 576, 576, p.xr.data() + (gr * nch_ + c) * 576);
                p.side[gr * nch_ + c] = v.side[v.unit(c, i, gr)];
            }
        return p;
    }
    std::array<StatePlane, 3> state_planes() { return {{plane_of(overlap_, 0), plane_of(vvec_, 1), plane_of(vfront_, 2)}}; }
    void put_state(const symaccel_batch_slot &slot) { store_state(state_planes(), slot); }
    void take_state(const symaccel_batch_slot &slot) { load_state(state_planes(), slot); }

private:
    std::size_t nch_, ngr_;
    int sr_;
    std::vector<float> overlap_, vvec_, in_;
    std::vector<std::int32_t> vfront_;
    std::vector<symaccel_mp3_side> side_;
};

// MPEG-1/2 Layer I and Layer II: one packet = one frame = 384 (Layer I) or 1152 (Layer II) frames per channel.  Per channel-packet:
// what the bit reader leaves -- the raw sample codes, sub-band major, and the allocation / scale-factor record (layer1/mod.rs:101-138,
// layer2/mod.rs:262-318; include/symaccel.h, symaccel_mpa12_decode) -- handed to the fused kernel, which dequantises, scales and runs the
// polyphase filterbank (layer1/mod.rs:142-194, layer2/mod.rs:320-384).  Two bytes per sample cross the link instead of four.  Chains are
// independent (an intensity-coded sub-band simply has the same codes in both channels), so streams of any channel count share a launch.
struct Mpa12 : CodecBase {
    using Sample = float;
    struct Params {
        int layer = SYMACCEL_MPA_LAYER2;
        std::size_t channels = 2;
    };
    struct Packet {
        std::uint64_t ts = 0;
        std::vector<std::uint16_t> codes;  // [channel][32][n_frames]
        std::vector<std::uint8_t> rec;     // [channel][record bytes]
    };
    explicit Mpa12(const Params &p)
        : layer_(p.layer), nch_(p.channels), nf_(p.layer == SYMACCEL_MPA_LAYER1 ? 12 : 36), rb_(symaccel_mpa12_record_bytes(p.layer)), vvec_(p.channels * 1024, 0.0f),
          vfront_(p.channels, 0) {
        if (rb_ == 0) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "mpa: invalid mpeg audio layer");
        if (nch_ < 1 || nch_ > 2) throw std::invalid_argument("Mpa12: one or two channels");
    }
    std::size_t channels() const { return nch_; }
    std::size_t packet_frames(std::size_t) const { return 32 * nf_; }
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t k) const { return (c * k + i) * 32 * nf_; }
    void reset_state() {  // MpaDecoder::reset: fresh State (SynthesisState::default(), decoder.rs:152-155)
        std::fill(vvec_.begin(), vvec_.end(), 0.0f);
        std::fill(vfront_.begin(), vfront_.end(), 0);
    }
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<float> &pcm) {
        const std::size_t k = batch.size();
        codes_.resize(nch_ * k * 32 * nf_);
        rec_.resize(nch_ * k * rb_);
        status_.assign(nch_ * k, 0);
        pcm.resize(nch_ * k * 32 * nf_);
        const BatchView v{codes_.data(), rec_.data(), k, nf_, rb_};
        for (std::size_t i = 0; i < k; ++i) put(v, i, batch[i]);
        ctx.mpa12_decode(layer_, codes_.data(), rec_.data(), vvec_.data(), vfront_.data(), pcm.data(), nch_, k, status_.data());
        for (std::uint8_t st : status_)
            if (st) throw std::invalid_argument("Mpa12: a record is out of range");  // (what the batcher's ticket says: SYMACCEL_ERR_INVALID_ARG)
    }
    static constexpr int kBatchKind = SYMACCEL_BATCH_MPA12_DECODE;
    static constexpr bool kDirect = true;
    int batch_param() const { return layer_; }
    std::size_t batch_chains(std::size_t) const { return nch_; }
    std::size_t batch_units(std::size_t k) const { return k; }
    struct BatchView {  // packet i of channel c is unit i of chain c
        std::uint16_t *codes = nullptr;
        std::uint8_t *rec = nullptr;
        std::size_t k = 0, nf = 0, rb = 0;
        std::uint16_t *codes_of(std::size_t c, std::size_t i) const { return codes + (c * k + i) * 32 * nf; }
        std::uint8_t *rec_of(std::size_t c, std::size_t i) const { return rec + (c * k + i) * rb; }
    };
    BatchView view(const symaccel_batch_slot &slot, std::size_t k) const {
        return BatchView{static_cast<std::uint16_t *>(slot.input[0]), static_cast<std::uint8_t *>(slot.input[1]), k, nf_, rb_};
    }
    void put(const BatchView &v, std::size_t i, const Packet &p) const {
        if (p.codes.size() != nch_ * 32 * nf_ || p.rec.size() != nch_ * rb_) throw std::invalid_argument("Mpa12: packet shape");
        for (std::size_t c = 0; c < nch_; ++c) {
            std::copy_n(p.codes.data() + c * 32 * nf_, 32 * nf_, v.codes_of(c, i));
            std::copy_n(p.rec.data() + c * rb_, rb_, v.rec_of(c, i));
        }
    }
    Packet extract(const BatchView &v, std::size_t i) const {
        Packet p;
        p.codes.resize(nch_ * 32 * nf_);
        p.rec.resize(nch_ * rb_);
        for (std::size_t c = 0; c < nch_; ++c) {
            std::copy_n(v.codes_of(c, i), 32 * nf_, p.codes.data() + c * 32 * nf_);
            std::copy_n(v.rec_of(c, i), rb_, p.rec.data() + c * rb_);
        }
        return p;
    }
    std::array<StatePlane, 2> state_planes() { return {{plane_of(vvec_, 0), plane_of(vfront_, 1)}}; }
    void put_state(const symaccel_batch_slot &slot) { store_state(state_planes(), slot); }
    void take_state(const symaccel_batch_slot &slot) { load_state(state_planes(), slot); }

private:
    int layer_;
    std::size_t nch_, nf_, rb_;
    std::vector<float> vvec_;
    std::vector<std::int32_t> vfront_;
    std::vector<std::uint16_t> codes_;
    std::vector<std::uint8_t> rec_, status_;
};

// The same Layer III packets one stage earlier: what the entropy decoder produces (layer3/mod.rs:393-420) -- the Huffman samples as
// int16, the GranuleChannel fields requantize reads, one stereo record per granule for a two-channel stream -- handed to
// symaccel_mp3_decode_pipelined, which runs requantize + joint stereo + the synthesis tail on the device (layer3/mod.rs:421-477).
// Half the bytes of Mp3's f32 spectra cross PCIe, and the host keeps neither POW43 nor the band loops.
struct Mp3Huffman : CodecBase {
    using Sample = float;
    struct Params {
        std::size_t channels = 2;  // 1, or 2 (one joint-stereo pair)
        std::size_t granules = 2;
        int sample_rate_idx = 0;
    };
    struct Packet {
        std::uint64_t ts = 0;
        std::vector<std::int16_t> quant;            // [granule][channel][576]
        std::vector<symaccel_mp3_requant> rq;       // [granule][channel]
        std::vector<symaccel_mp3_stereo> stereo;    // [granule] (two-channel streams)
        std::vector<symaccel_mp3_side> side;        // [granule][channel], rzero as it is AFTER stereo (stereo.rs:549-553)
    };
    explicit Mp3Huffman(const Params &p)
        : nch_(p.channels), ngr_(p.granules), sr_(p.sample_rate_idx), overlap_(p.channels * 576, 0.0f), vvec_(p.channels * 1024, 0.0f),
          vfront_(p.channels, 0) {
        if (p.channels < 1 || p.channels > 2) throw std::invalid_argument("Mp3Huffman: one or two channels");
    }
    std::size_t channels() const { return nch_; }
    std::size_t packet_frames(std::size_t) const { return 576 * ngr_; }
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t k) const { return (c * k + i) * 576 * ngr_; }
    void reset_state() {
        std::fill(overlap_.begin(), overlap_.end(), 0.0f);
        std::fill(vvec_.begin(), vvec_.end(), 0.0f);
        std::fill(vfront_.begin(), vfront_.end(), 0);
    }
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<float> &pcm) {
        const std::size_t k = batch.size(), g = k * ngr_;
        q_.resize(nch_ * g * 576);
        rq_.resize(nch_ * g);
        side_.resize(nch_ * g);
        st_.resize(nch_ == 2 ? g : 0);
        pcm.resize(nch_ * g * 576);
        const BatchView v{q_.data(), rq_.data(), side_.data(), nch_ == 2 ? st_.data() : nullptr, k, nch_, ngr_};  // (mono: no stereo plane)
        for (std::size_t i = 0; i < k; ++i) put(v, i, batch[i]);
        const std::int32_t pair[2] = {0, 1};
        check(symaccel_mp3_decode_pipelined(ctx.raw(), q_.data(), rq_.data(), nch_ == 2 ? pair : nullptr, v.stereo,
                                            nch_ == 2 ? 1 : 0, side_.data(), sr_, overlap_.data(), vvec_.data(), vfront_.data(), pcm.data(), nch_, g, 0),
              ctx.raw());
    }

    static constexpr int kBatchKind = SYMACCEL_BATCH_MP3_DECODE;  // one stream per submission: exactly what this codec is
    static constexpr bool kDirect = true;
    int batch_param() const { return sr_; }
    std::size_t batch_chains(std::size_t) const { return nch_; }
    std::size_t batch_units(std::size_t k) const { return k * ngr_; }
    struct BatchView {  // granule gr of packet i of channel c is unit i * ngr + gr of chain c; the stereo records are per granule of the STREAM
        std::int16_t *quant = nullptr;
        symaccel_mp3_requant *rq = nullptr;
        symaccel_mp3_side *side = nullptr;
        symaccel_mp3_stereo *stereo = nullptr;
        std::size_t k = 0, nch = 0, ngr = 0;
        std::size_t unit(std::size_t c, std::size_t i, std::size_t gr) const { return c * k * ngr + i * ngr + gr; }
    };
    BatchView view(const symaccel_batch_slot &slot, std::size_t k) const {
        return BatchView{static_cast<std::int16_t *>(slot.input[0]), static_cast<symaccel_mp3_requant *>(slot.input[1]),
                         static_cast<symaccel_mp3_side *>(slot.input[2]), static_cast<symaccel_mp3_stereo *>(slot.input[3]), k, nch_, ngr_};
    }
    static void put(const BatchView &v, std::size_t i, const Packet &p) {
        if (p.quant.size() != v.ngr * v.nch * 576 || p.rq.size() != v.ngr * v.nch || p.side.size() != v.ngr * v.nch || p.stereo.size() != (v.nch == 2 ? v.ngr : 0))
            throw std::invalid_argument("Mp3Huffman: packet shape");
        for (std::size_t gr = 0; gr < v.ngr; ++gr) {
            for (std::size_t c = 0; c < v.nch; ++c) {
                const std::size_t dst = v.unit(c, i, gr);
                std::copy_n(p.quant.data() + (gr * v.nch + c) * 576, 576, v.quant + dst * 576);
                v.rq[dst] = p.rq[gr * v.nch + c];
                v.side[dst] = p.side[gr * v.nch + c];
            }
            // a mono stream has no stereo records: a slot's plane (it has one whatever the channel count) stays zeroed, decode_batch has none
            if (v.nch == 2) v.stereo[i * v.ngr + gr] = p.stereo[gr];
            else if (v.stereo) std::memset(&v.stereo[i * v.ngr + gr], 0, sizeof(symaccel_mp3_stereo));
        }
    }
    Packet extract(const BatchView &v, std::size_t i) const {
        Packet p;
        p.quant.resize(ngr_ * nch_ * 576);
        p.rq.resize(ngr_ * nch_);
        p.side.resize(ngr_ * nch_);
        p.stereo.resize(nch_ == 2 ? ngr_ : 0);
        for (std::size_t gr = 0; gr < ngr_; ++gr) {
            for (std::size_t c = 0; c < nch_; ++c) {
                const std::size_t src = v.unit(c, i, gr);
                std::copy_n(v.quant + src * 576, 576, p.quant.data() + (gr * nch_ + c) * 576);
                p.rq[gr * nch_ + c] = v.rq[src];
                p.side[gr * nch_ + c] = v.side[src];
            }
            if (nch_ == 2) p.stereo[gr] = v.stereo[i * ngr_ + gr];
        }
        return p;
    }
    std::array<StatePlane, 3> state_planes() { return {{plane_of(overlap_, 0), plane_of(vvec_, 1), plane_of(vfront_, 2)}}; }
    void put_state(const symaccel_batch_slot &slot) { store_state(state_planes(), slot); }
    void take_state(const symaccel_batch_slot &slot) { load_state(state_planes(), slot); }

private:
    std::size_t nch_, ngr_;
    int sr_;
    std::vector<float> overlap_, vvec_;
    std::vector<std::int32_t> vfront_;
    std::vector<std::int16_t> q_;
    std::vector<symaccel_mp3_requant> rq_;
    std::vector<symaccel_mp3_stereo> st_;
    std::vector<symaccel_mp3_side> side_;
};

// Vorbis: one packet = one audio block of the size its mode's block flag selects.  What the CPU side hands over per
// channel: floor x residue, the n / 2 lines DspChannel::synth receives (lib.rs:282-331).  A packet yields
// (prev_n + n) / 4 frames -- none for the first block after a reset (dsp.rs:77-80) -- so the batch's PCM is packed
// (include/symaccel.h, "Vorbis") and the per-packet spans are what publish() asks for.
struct Vorbis : CodecBase {
    using Sample = float;
    struct Params {
        std::size_t channels = 2;
        int bs0_exp = 8, bs1_exp = 11;
    };
    struct Packet {
        std::uint64_t ts = 0;
        bool long_block = false;
        std::vector<float> spectra;  // [channel][n / 2]
    };
    explicit Vorbis(const Params &p)
        : nch_(p.channels), e0_(p.bs0_exp), e1_(p.bs1_exp), prev_(p.channels, -1), overlap_(p.channels * ((std::size_t)1 << (p.bs1_exp - 1)), 0.0f) {}
    std::size_t channels() const { return nch_; }
    std::size_t packet_frames(std::size_t i) const { return emits_[i] ? off_[i + 1] - off_[i] : 0; }
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t) const { return c * stride_ + off_[i]; }
    void reset_state() {  // Dsp::reset (dsp.rs:45-56): no block to lap with, overlap zeroed
        std::fill(prev_.begin(), prev_.end(), -1);
        std::fill(overlap_.begin(), overlap_.end(), 0.0f);
    }
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<float> &pcm) {
        const std::size_t k = batch.size();
        std::size_t lines = 0, samples = 0;
        layout(batch, &lines, &samples);
        stride_ = samples;
        in_.resize(nch_ * lines);
        flags_.resize(nch_ * k);
        pcm.assign(nch_ * samples, 0.0f);
        gather(batch, in_.data(), lines, flags_.data());
        check(symaccel_vorbis_synth(ctx.raw(), e0_, e1_, in_.data(), lines, flags_.data(), prev_.data(), overlap_.data(), pcm.data(), samples,
                                    nch_, k),
              ctx.raw());
    }
    // the cross-stream batcher's view: every chain's planes at their largest (k * bs1 / 2), the packed data at the front -- so that
    // streams with different block flags share a launch (SYMACCEL_BATCH_VORBIS_SYNTH)
    static constexpr int kBatchKind = SYMACCEL_BATCH_VORBIS_SYNTH;  // (not kDirect: the packed layout depends on every packet's block flag)
    int batch_param() const { return e0_ | (e1_ << 8); }
    std::size_t batch_chains(std::size_t) const { return nch_; }  // a submission of k packets: nch chains of k units
    std::size_t batch_units(std::size_t k) const { return k; }
    void fill_slot(const std::vector<Packet> &batch, const symaccel_batch_slot &slot) {
        const std::size_t k = batch.size(), cap = k << (e1_ - 1);
        // (the batch being handed out keeps its offsets until this one is collected: the submitted batch's layout waits in next_*)
        std::vector<std::size_t> cur_off, cur_spec;
        std::vector<bool> cur_emits;
        cur_off.swap(off_);
        cur_spec.swap(spec_off_);
        cur_emits.swap(emits_);
        std::size_t lines = 0, samples = 0;
        layout(batch, &lines, &samples);
        gather(batch, static_cast<float *>(slot.input[0]), cap, static_cast<std::uint8_t *>(slot.input[1]));
        next_off_.swap(off_);
        next_emits_.swap(emits_);
        next_stride_ = cap;
        off_.swap(cur_off);
        spec_off_.swap(cur_spec);
        emits_.swap(cur_emits);
        store_state(state_planes(), slot);
    }
    std::array<StatePlane, 2> state_planes() { return {{plane_of(prev_, 0), plane_of(overlap_, 1)}}; }
    void take_state(const symaccel_batch_slot &slot) {
        load_state(state_planes(), slot);
        off_.swap(next_off_);
        emits_.swap(next_emits_);
        stride_ = next_stride_;
    }

private:
    // packed offsets of the batch's blocks inside a chain: spec_off_[i] lines, off_[i] samples (a first block owns n / 2 untouched slots)
    void layout(const std::vector<Packet> &batch, std::size_t *lines_out, std::size_t *samples_out) {
        const std::size_t k = batch.size();
        const std::size_t bs[2] = {(std::size_t)1 << e0_, (std::size_t)1 << e1_};
        spec_off_.assign(k, 0);
        off_.assign(k + 1, 0);
        emits_.assign(k, false);
        std::size_t lines = 0, samples = 0;
        int prev = prev_[0];
        for (std::size_t i = 0; i < k; ++i) {
            const std::size_t n = bs[batch[i].long_block ? 1 : 0];
            if (batch[i].spectra.size() != nch_ * n / 2) throw std::invalid_argument("Vorbis: packet shape");
            spec_off_[i] = lines;
            off_[i] = samples;
            emits_[i] = prev >= 0;
            lines += n / 2;
            samples += prev >= 0 ? (bs[prev] + n) / 4 : n / 2;
            prev = batch[i].long_block ? 1 : 0;
        }
        off_[k] = samples;
        *lines_out = lines;
        *samples_out = samples;
    }
    void gather(const std::vector<Packet> &batch, float *in, std::size_t spec_stride, std::uint8_t *flags) const {
        const std::size_t k = batch.size();
        const std::size_t bs[2] = {(std::size_t)1 << e0_, (std::size_t)1 << e1_};
        for (std::size_t i = 0; i < k; ++i) {
            const std::size_t half = bs[batch[i].long_block ? 1 : 0] / 2;
            for (std::size_t c = 0; c < nch_; ++c) {
                std::copy_n(batch[i].spectra.data() + c * half, half, in + c * spec_stride + spec_off_[i]);
                flags[c * k + i] = batch[i].long_block ? 1 : 0;
            }
        }
    }
    std::size_t nch_;
    int e0_, e1_;
    std::vector<std::int32_t> prev_;
    std::vector<float> overlap_, in_;
    std::vector<std::uint8_t> flags_;
    std::vector<std::size_t> off_, spec_off_, next_off_;
    std::vector<bool> emits_, next_emits_;
    std::size_t stride_ = 0, next_stride_ = 0;
};

// FLAC: one packet = one frame = one subframe per channel.  What the CPU side (frame / subframe headers, Rice decode:
// flac/decoder.rs:381-660) hands over per channel: `blocksize` words -- the warm-up samples followed by the residuals,
// exactly what fixed_predict / lpc_predict receive --, the subframe descriptor and its quantised coefficients, and per
// frame the channel assignment.  The predictor restore of every subframe of the batch runs in one device call
// (decoder.rs:663-752), then the stereo decorrelation and the `<< (32 - bps)` of decoder.rs:199-242.  FLAC carries no
// state from frame to frame, so reset() has nothing to zero; block sizes may differ from packet to packet (the last
// frame; variable-block-size streams): every subframe gets a slot of the batch's largest block size.
struct Flac : CodecBase {
    using Sample = std::int32_t;
    struct Params {
        std::size_t channels = 2;
        std::uint32_t bits_per_sample = 16;
        std::size_t max_blocksize = 4096;  // STREAMINFO's maximum block size: the slot every subframe gets with the batcher
        bool verify = false;               // AudioDecoderOptions::verify: hash the decoded audio (validate.rs:25-75) ...
        std::optional<std::array<std::uint8_t, 16>> expected_md5;  // ... and compare with STREAMINFO's digest, if it has one (decoder.rs:272-308)
    };
    struct Packet {
        std::uint64_t ts = 0;
        std::size_t blocksize = 0;
        std::vector<std::int32_t> words;        // [channel][blocksize]
        std::vector<symaccel_flac_desc> desc;   // [channel]
        std::vector<std::int32_t> coeffs;       // [channel][32], reference order (decoder.rs:716-752)
        std::uint8_t pair_mode = 0;             // 0 independent, 1 left/side, 2 mid/side, 3 right/side (two-channel frames)
    };
    explicit Flac(const Params &p) : nch_(p.channels), shift_(32u - p.bits_per_sample), max_bs_(p.max_blocksize), expected_(p.expected_md5) {
        if (p.channels == 0 || p.bits_per_sample == 0 || p.bits_per_sample > 32 || p.max_blocksize == 0 || p.max_blocksize > 65535)
            throw std::invalid_argument("Flac: parameters");
        symaccel_md5_init(&published_);
        chain_end_ = published_;
        set_verify(p.verify);
    }
    // Verification (the STREAMINFO MD5): the batches go through the verify forms of the kind -- restore, then one MD5 wavefront per
    // stream in the same launch, the state after every frame coming back as a checkpoint.  `published_` is the state after the last
    // packet handed out, `chain_end_` the state after the last frame of the most recently computed batch (what the next batch starts
    // from); a seek or a skip drops the difference (the reference's reset() leaves its validator alone, decoder.rs:254-256).
    void set_verify(bool on) {
        if (on && nch_ > 8) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "flac: verification of more than 8 channels");
        verify_ = on;
    }
    void set_replaying(bool on) { replaying_ = on; }
    void published(std::size_t i) {
        if (verify_ && i < cps_.size()) published_ = cps_[i];
    }
    void rewind() { chain_end_ = published_; }
    FinalizeResult finalize_result() {
        FinalizeResult r;
        if (verify_ && expected_) {  // (no digest in STREAMINFO: the reference only warns, decoder.rs:302-304)
            std::array<std::uint8_t, 16> got{};
            symaccel_md5_digest(&published_, got.data());
            r.verify_ok = got == *expected_;
        }
        return r;
    }
    std::array<std::uint8_t, 16> md5_so_far() const {  // the digest over the packets handed out so far
        std::array<std::uint8_t, 16> got{};
        symaccel_md5_digest(&published_, got.data());
        return got;
    }
    // With the batcher (SYMACCEL_BATCH_FLAC_RESTORE) a chain is ONE SUBFRAME and the unit count is the stream's maximum block size, so
    // the batches of every FLAC stream with that block size share launches whatever their lengths; a two-channel stream takes the
    // fused form (param 0x100 | shift: decorrelation and left-justification in the restore kernel's write-back, decoder.rs:199-242),
    // every other layout the plain one with the shift on the host.  Verifying, the same split: 0x300 | shift (the finishing MD5 kernel
    // leaves the pair decorrelated and left-justified) for two channels, 0x200 otherwise.
    static constexpr int kBatchKind = SYMACCEL_BATCH_FLAC_RESTORE;
    static constexpr bool kVerifies = true;
    void attach(Batcher &b) { narrow_ok_ = b.narrow_input(), rows_ok_ = b.input_mode() == Batcher::InputMode::Rows; }
    // The input format of a batch (LookaheadDecoder asks before it reserves: the format belongs to the reservation): int16_t when EVERY
    // warm-up sample and residual of the batch fits -- the 16-bit streams, but for a side channel's 17-bit warm-up here and there --, else
    // the native words exactly as before.  Per batch; nothing else about the decoder depends on it.  Batcher::InputMode::Rows: a width per
    // row, which fill_slot() finds as it packs -- nothing to look at here.
    int input_format(const std::vector<Packet> &batch) {
        narrow_next_ = false;
        if ((rows_next_ = rows_ok_)) return SYMACCEL_IN_FMT_ROWS;
        std::uint32_t miss = 0;
        if (narrow_ok_)
            for (const Packet &p : batch)
                for (const std::int32_t v : p.words) miss |= (std::uint32_t)v ^ (std::uint32_t)(std::int32_t)(std::int16_t)v;
        narrow_next_ = narrow_ok_ && miss == 0;
        ++(narrow_next_ ? narrow_batches_ : wide_batches_);
        return narrow_next_ ? SYMACCEL_FMT_S16 : 0;
    }
    std::size_t narrow_batches() const { return narrow_batches_; }
    std::size_t wide_batches() const { return wide_batches_; }
    std::array<std::size_t, 3> rows_sent() const { return rows_sent_; }
    std::size_t plane0_bytes() const { return plane0_bytes_; }
    int batch_param() const {
        if (hashing()) return (nch_ == 2 ? (int)(0x300u | shift_) : 0x200) | (int)((nch_ - 1) << 12);
        return nch_ == 2 ? (int)(0x100u | shift_) : 0;
    }
    std::size_t batch_chains(std::size_t k) const { return k * nch_; }
    std::size_t batch_units(std::size_t) const { return max_bs_; }
    void fill_slot(const std::vector<Packet> &batch, const symaccel_batch_slot &slot) {
        const std::size_t k = batch.size();
        std::int32_t *words = static_cast<std::int32_t *>(slot.input[0]);
        symaccel_flac_desc *desc = static_cast<symaccel_flac_desc *>(slot.input[1]);
        std::int32_t *coeffs = static_cast<std::int32_t *>(slot.input[2]);
        next_lens_.assign(k, 0);
        for (std::size_t i = 0; i < k; ++i) {
            const Packet &p = batch[i];
            check_shape(p, max_bs_);
            next_lens_[i] = p.blocksize;
            for (std::size_t c = 0; c < nch_; ++c) {
                if (rows_next_) {  // the row at the narrowest width that holds it, at its native offset; zero is zero at any width
                    const std::size_t r = i * nch_ + c;
                    std::uint8_t *row = static_cast<std::uint8_t *>(slot.input[0]) + r * max_bs_ * 4;
                    const int w = symaccel_host_pack_row(p.words.data() + c * p.blocksize, row, p.blocksize);
                    if (w < 2 || w > 4) throw std::logic_error("Flac: symaccel_host_pack_row");
                    std::fill(row + p.blocksize * (std::size_t)w, row + max_bs_ * (std::size_t)w, (std::uint8_t)0);
                    static_cast<std::uint8_t *>(slot.input[5])[r] = (std::uint8_t)w;
                    ++rows_sent_[(std::size_t)w - 2];
                    plane0_bytes_ += max_bs_ * (std::size_t)w;
                } else if (narrow_next_) {  // (input_format() found that every word fits: packed straight into the slot)
                    std::int16_t *row = static_cast<std::int16_t *>(slot.input[0]) + (i * nch_ + c) * max_bs_;
                    if (!symaccel_host_narrow_s16(p.words.data() + c * p.blocksize, row, p.blocksize)) throw std::logic_error("Flac: a narrow batch with a wide word");
                    std::fill(row + p.blocksize, row + max_bs_, (std::int16_t)0);
                } else {
                    std::int32_t *row = words + (i * nch_ + c) * max_bs_;
                    std::copy_n(p.words.data() + c * p.blocksize, p.blocksize, row);
                    std::fill(row + p.blocksize, row + max_bs_, 0);  // (restoring the padding is harmless: it is never published)
                }
                desc[i * nch_ + c] = p.desc[c];
                std::copy_n(p.coeffs.data() + c * 32, 32, coeffs + (i * nch_ + c) * 32);
            }
            if (hashing()) static_cast<symaccel_flac_md5_frame *>(slot.input[3])[i] = md5_frame(p);
            else if (nch_ == 2) static_cast<std::uint8_t *>(slot.input[3])[i] = p.pair_mode;
        }
        if (!rows_next_) plane0_bytes_ += k * nch_ * max_bs_ * (narrow_next_ ? 2 : 4);
        if (hashing()) static_cast<symaccel_md5_state *>(slot.state[0])[0] = chain_end_;
    }
    void take_state(const symaccel_batch_slot &slot) {
        lens_.swap(next_lens_);
        stride_ = max_bs_;
        if (hashing()) {  // entry f: the state after frame f
            const symaccel_md5_state *st = static_cast<const symaccel_md5_state *>(slot.state[0]);
            cps_.assign(st, st + lens_.size());
            if (!cps_.empty()) chain_end_ = cps_.back();
        } else {
            cps_.clear();
        }
        if (nch_ != 2) {  // decoder.rs:239-242 (the two-channel form did it on the device)
            std::int32_t *words = static_cast<std::int32_t *>(slot.out);
            for (std::size_t i = 0; i < slot.out_bytes / 4; ++i) words[i] = (std::int32_t)((std::uint32_t)words[i] << shift_);
        }
    }
    std::size_t channels() const { return nch_; }
    bool device_output_is_final() const { return nch_ == 2; }  // (set_output: other layouts are left-justified on the host, take_state)
    std::size_t packet_frames(std::size_t i) const { return lens_[i]; }
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t) const { return (i * nch_ + c) * stride_; }
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<std::int32_t> &pcm) {
        const std::size_t k = batch.size();
        stride_ = 0;
        lens_.assign(k, 0);
        for (std::size_t i = 0; i < k; ++i) {
            const Packet &p = batch[i];
            check_shape(p, 65535);
            lens_[i] = p.blocksize;
            stride_ = std::max(stride_, p.blocksize);
        }
        pcm.assign(k * nch_ * stride_, 0);
        desc_.resize(k * nch_);
        coeffs_.resize(k * nch_ * 32);
        modes_.resize(k);
        for (std::size_t i = 0; i < k; ++i) {
            const Packet &p = batch[i];
            for (std::size_t c = 0; c < nch_; ++c) {
                std::copy_n(p.words.data() + c * p.blocksize, p.blocksize, pcm.data() + (i * nch_ + c) * stride_);
                desc_[i * nch_ + c] = p.desc[c];
                // a slot longer than its block: the restore runs over `stride_` words, the tail is zero residual and is never published
                std::copy_n(p.coeffs.data() + c * 32, 32, coeffs_.data() + (i * nch_ + c) * 32);
            }
            modes_[i] = p.pair_mode;
        }
        check(symaccel_flac_restore(ctx.raw(), pcm.data(), desc_.data(), coeffs_.data(), k * nch_, stride_), ctx.raw());
        cps_.clear();
        if (hashing() && k) {  // the restored words, before the decorrelation and the shift: what the reference hashes (decoder.rs:231-234)
            frames_.resize(k);
            for (std::size_t i = 0; i < k; ++i) frames_[i] = md5_frame(batch[i]);
            cps_.resize(k);
            check(symaccel_flac_md5(ctx.raw(), pcm.data(), stride_, frames_.data(), k, (int)nch_, (int)bytes_per_sample(), &chain_end_, cps_.data()), ctx.raw());
        }
        if (nch_ == 2) {
            // pair i = (channel 0, channel 1) of packet i: rows 2 i and 2 i + 1 of the batch
            ch0_.resize(k * stride_);
            ch1_.resize(k * stride_);
            for (std::size_t i = 0; i < k; ++i) {
                std::copy_n(pcm.data() + (2 * i) * stride_, stride_, ch0_.data() + i * stride_);
                std::copy_n(pcm.data() + (2 * i + 1) * stride_, stride_, ch1_.data() + i * stride_);
            }
            check(symaccel_flac_decorrelate(ctx.raw(), modes_.data(), ch0_.data(), ch1_.data(), k, stride_, shift_), ctx.raw());
            for (std::size_t i = 0; i < k; ++i) {
                std::copy_n(ch0_.data() + i * stride_, stride_, pcm.data() + (2 * i) * stride_);
                std::copy_n(ch1_.data() + i * stride_, stride_, pcm.data() + (2 * i + 1) * stride_);
            }
        } else {
            for (std::int32_t &v : pcm) v = (std::int32_t)((std::uint32_t)v << shift_);  // decoder.rs:239-242
        }
    }

private:
    // a packet's shape; `limit`: the longest block its destination takes (the slot's rows with the batcher, the block-size field without)
    void check_shape(const Packet &p, std::size_t limit) const {
        if (p.blocksize == 0 || p.blocksize > limit || p.words.size() != nch_ * p.blocksize || p.desc.size() != nch_ || p.coeffs.size() != nch_ * 32 ||
            p.pair_mode > 3 || (p.pair_mode != 0 && nch_ != 2))
            throw std::invalid_argument("Flac: packet shape");
    }
    bool hashing() const { return verify_ && !replaying_; }
    unsigned bytes_per_sample() const { return (32u - shift_ + 7) / 8; }  // validate.rs:39-45
    symaccel_flac_md5_frame md5_frame(const Packet &p) const {
        return symaccel_flac_md5_frame{(std::uint16_t)p.blocksize, p.pair_mode, (std::uint8_t)bytes_per_sample()};
    }
    std::size_t nch_;
    std::uint32_t shift_;
    std::size_t max_bs_;
    std::optional<std::array<std::uint8_t, 16>> expected_;
    bool verify_ = false, replaying_ = false;
    bool narrow_ok_ = false, narrow_next_ = false;  // the batcher's setting (attach); the format of the batch being submitted
    std::size_t narrow_batches_ = 0, wide_batches_ = 0;
    bool rows_ok_ = false, rows_next_ = false;  // Batcher::InputMode::Rows (attach); the batch being submitted carries a width per row
    std::array<std::size_t, 3> rows_sent_{{0, 0, 0}};
    std::size_t plane0_bytes_ = 0;
    symaccel_md5_state published_{}, chain_end_{};
    std::vector<symaccel_md5_state> cps_;  // the state after every packet of the current batch
    std::vector<symaccel_flac_md5_frame> frames_;
    std::size_t stride_ = 0;
    std::vector<std::size_t> lens_, next_lens_;
    std::vector<symaccel_flac_desc> desc_;
    std::vector<std::int32_t> coeffs_, ch0_, ch1_;
    std::vector<std::uint8_t> modes_;
};

// ADPCM (symphonia-codec-adpcm): MS, IMA WAV, IMA QT; mono and stereo.  A packet is block_dur / frames_per_block blocks back to back
// (lib.rs:122-168) and there is NO CPU side: the packet's bytes go up as they are, the whole numeric decode runs on the device
// (csrc/adpcm.hip).  Nothing is carried from packet to packet (lib.rs:217-219), so reset() has nothing to zero and a skipped packet needs
// no replay.  With the batcher (SYMACCEL_BATCH_ADPCM_DECODE) a chain is ONE BLOCK and every packet gets `max_frames_per_packet /
// frames_per_block` chains (a shorter last packet leaves zero blocks behind it, never published), so the packets of every stream of one
// codec, channel count and block size share launches.  The device writes pcm[block][channel][fpb]; the trait's planes are
// [channel][block * fpb + frame], so a stereo packet of several blocks is re-packed in the slot on the host (take_state).  A delivered
// format needs no re-pack: the kernel writes [block][frame][channel] and a packet's blocks follow one another.
struct Adpcm : CodecBase {
    using Sample = std::int32_t;
    struct Params {
        int codec = SYMACCEL_ADPCM_MS;  // SYMACCEL_ADPCM_*
        std::size_t channels = 2;
        std::size_t frames_per_block = 0;       // AudioCodecParameters::frames_per_block (lib.rs:84-86)
        std::size_t max_frames_per_packet = 0;  // ... ::max_frames_per_packet (lib.rs:79-82)
    };
    struct Packet {
        std::uint64_t ts = 0;
        std::size_t block_dur = 0;         // frames (packet.block_dur(), lib.rs:131)
        std::vector<std::uint8_t> data;    // at least block_dur / frames_per_block blocks; what follows them is ignored, as in the reference
    };
    // Error{Unsupported} for the shapes the device decoder leaves to the decoder below (symaccel_adpcm_block_bytes == 0)
    explicit Adpcm(const Params &p)
        : codec_(p.codec), nch_(p.channels), fpb_(p.frames_per_block), bytes_(symaccel_adpcm_block_bytes(p.codec, p.channels, p.frames_per_block)),
          bpp_(p.frames_per_block ? p.max_frames_per_packet / p.frames_per_block : 0) {
        if (bytes_ == 0) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "adpcm: a shape the device decoder refuses");
        if (bpp_ == 0) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "adpcm: maximum frames per packet is required");
    }
    static constexpr int kBatchKind = SYMACCEL_BATCH_ADPCM_DECODE;
    static constexpr bool kBlockInterleave = true;
    void set_output_format(SampleFormat f) { native_ = f == SampleFormat::Native; }
    int batch_param() const { return codec_ | (int)(nch_ << 8); }
    std::size_t batch_chains(std::size_t k) const { return k * bpp_; }
    std::size_t batch_units(std::size_t) const { return bytes_; }
    std::size_t block_bytes() const { return bytes_; }
    // The packet's block count, and what the reference's readers would make of it, in their order (lib.rs:131-165 over io/buf_reader.rs):
    // block after block, the preamble bytes as they are read -- an MS block predictor above 6 is Unsupported (codec_ms.rs:25-29, 47-63), an
    // IMA WAV step index above 88 a DecodeError (codec_ima_wav.rs:14-25; the C++ Error has no such kind: Kind::IoError carrying the status
    // SYMACCEL_ERR_DECODE is how this header spells it, as check() does) --, a read past the end of the packet the I/O error of BufReader.
    std::size_t inspect(const Packet &p, std::optional<Error> *err) const {
        const std::size_t n = p.block_dur / fpb_;
        if (n > bpp_) throw std::invalid_argument("Adpcm: a packet longer than max_frames_per_packet");
        err->reset();
        for (std::size_t j = 0; j < n && !*err; ++j) {
            const std::size_t at = j * bytes_, left = p.data.size() > at ? p.data.size() - at : 0;
            const std::uint8_t *b = p.data.data() + at;
            for (std::size_t c = 0; c < nch_ && !*err; ++c) {
                if (codec_ == SYMACCEL_ADPCM_MS) {
                    if (left <= c) err->emplace(Error::Kind::IoError, SYMACCEL_ERR_DEVICE, "adpcm: buffer underrun");
                    else if (b[c] > 6) err->emplace(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "adpcm: block predictor exceeds range");
                } else if (codec_ == SYMACCEL_ADPCM_IMA_WAV) {
                    if (left < 4 * c + 3) err->emplace(Error::Kind::IoError, SYMACCEL_ERR_DEVICE, "adpcm: buffer underrun");
                    else if (b[4 * c + 2] > 88) err->emplace(Error::Kind::IoError, SYMACCEL_ERR_DECODE, "adpcm (ima): invalid step index");
                    else if (left < 4 * c + 4) err->emplace(Error::Kind::IoError, SYMACCEL_ERR_DEVICE, "adpcm: buffer underrun");
                }
            }
            if (!*err && left < bytes_) err->emplace(Error::Kind::IoError, SYMACCEL_ERR_DEVICE, "adpcm: buffer underrun");
        }
        return n;
    }
    const Error *packet_error(std::size_t i) const { return i < errors_.size() && errors_[i] ? &*errors_[i] : nullptr; }
    // packet i's blocks into `rows` (bpp slots of it): a packet with an error of its own, and the slots behind a short packet, run as zero
    // blocks (an accepted preamble, silence), which nobody is shown
    std::size_t place(const Packet &p, std::uint8_t *rows, std::size_t slots, std::optional<Error> *err) const {
        const std::size_t n = inspect(p, err), good = *err ? 0 : n;
        std::copy_n(p.data.data(), good * bytes_, rows);
        std::fill(rows + good * bytes_, rows + slots * bytes_, 0);
        return n;
    }
    void fill_slot(const std::vector<Packet> &batch, const symaccel_batch_slot &slot) {
        std::uint8_t *rows = static_cast<std::uint8_t *>(slot.input[0]);
        next_blocks_.assign(batch.size(), 0);
        next_errors_.assign(batch.size(), std::nullopt);
        for (std::size_t i = 0; i < batch.size(); ++i) next_blocks_[i] = place(batch[i], rows + i * bpp_ * bytes_, bpp_, &next_errors_[i]);
    }
    void take_state(const symaccel_batch_slot &slot) {
        blocks_.swap(next_blocks_);
        errors_.swap(next_errors_);
        stride_ = bpp_;
        if (native_ && nch_ == 2 && bpp_ > 1) repack(static_cast<std::int32_t *>(slot.out), blocks_.size(), bpp_);
    }
    std::size_t channels() const { return nch_; }
    std::size_t packet_frames(std::size_t i) const { return blocks_[i] * fpb_; }
    // native: packet i's channel c is [block * fpb + frame] at (i * nch + c) * stride * fpb; a format: channel 0 names the packet's first sample
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t) const { return (i * nch_ + (native_ ? c : 0)) * stride_ * fpb_; }
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<std::int32_t> &pcm) {
        const std::size_t k = batch.size();
        blocks_.assign(k, 0);
        errors_.assign(k, std::nullopt);
        stride_ = bpp_;
        rows_.assign(k * stride_ * bytes_, 0);
        for (std::size_t i = 0; i < k; ++i) blocks_[i] = place(batch[i], rows_.data() + i * stride_ * bytes_, stride_, &errors_[i]);
        pcm.assign(k * stride_ * nch_ * fpb_, 0);
        if (k * stride_ == 0) return;
        ctx.adpcm_decode(rows_.data(), bytes_, k * stride_, codec_, nch_, fpb_, pcm.data(), SampleFormat::Native, nullptr);
        if (nch_ == 2 && stride_ > 1) repack(pcm.data(), k, stride_);
    }

private:
    // [packet][block][channel][fpb] -> [packet][channel][block][fpb], packet by packet
    void repack(std::int32_t *pcm, std::size_t k, std::size_t blocks) {
        tmp_.resize(blocks * nch_ * fpb_);
        for (std::size_t i = 0; i < k; ++i) {
            std::int32_t *p = pcm + i * blocks * nch_ * fpb_;
            std::copy_n(p, tmp_.size(), tmp_.data());
            for (std::size_t c = 0; c < nch_; ++c)
                for (std::size_t j = 0; j < blocks; ++j) std::copy_n(tmp_.data() + (j * nch_ + c) * fpb_, fpb_, p + (c * blocks + j) * fpb_);
        }
    }
    int codec_;
    std::size_t nch_, fpb_, bytes_, bpp_;
    std::size_t stride_ = 0;  // blocks every packet of the current batch occupies
    bool native_ = true;
    std::vector<std::size_t> blocks_, next_blocks_;
    std::vector<std::optional<Error>> errors_, next_errors_;  // per packet of the batch: what decode() throws when its turn comes
    std::vector<std::uint8_t> rows_;
    std::vector<std::int32_t> tmp_;
};

// PCM and G.711 (symphonia-codec-pcm): the twenty codecs of PcmDecoder.  Like ADPCM there is NO CPU side: the packet's bytes go up as
// they are and csrc/pcm_decode.hip does the de-interleave, byte order, shift, log expansion and conversion.  Nothing is carried from
// packet to packet (lib.rs:415-417) and no packet can fail (lib.rs:328: the render's Result is discarded).
//
// A packet is floor(len / (coded bytes * channels)) frames (lib.rs:320), so the packets of a look-ahead batch may differ in length.  A
// batch is ONE call (one batcher submission): every packet is a chain of `units` frames, `units` being the frames of the batch's longest
// packet; a shorter packet is followed by zero bytes, decodes them as well, and publishes its own frame count -- streams cut their packets
// to one size, so only the last packet of a stream pays for it, and with the batcher (SYMACCEL_BATCH_PCM_DECODE) the batches of every
// stream of one codec, channel count, shift and frame count share launches.  A batch of empty packets is a submission of 0 frames.
//
// The native planes are the reference's buffer sample type as Rust holds it (symaccel_pcm_native_bytes: 1, 2, 4 or 8 bytes; i24 / u24 in a
// 32-bit word), so Sample is a byte: `planes[c]` points at `frames * native_bytes()` bytes, to be read as variant()'s type.
struct Pcm : CodecBase {
    using Sample = std::uint8_t;
    struct Params {  // AudioCodecParameters (codecs/audio.rs:300-400): what PcmDecoder::try_new reads
        int codec = SYMACCEL_PCM_S16LE;  // SYMACCEL_PCM_*; anything else is a codec the reference's decoder does not take either
        std::optional<std::uint32_t> sample_rate;
        std::optional<std::size_t> channels;
        std::optional<std::uint32_t> bits_per_sample, bits_per_coded_sample;
        std::optional<std::uint64_t> max_frames_per_packet;  // (the reference pre-allocates with it; nothing here depends on it)
    };
    struct Packet {
        std::uint64_t ts = 0;
        std::vector<std::uint8_t> data;
    };
    // The checks of PcmDecoder::try_new in their order with their error kinds (lib.rs:220-303; the C++ Error has no DecodeError kind:
    // Kind::IoError carrying the status SYMACCEL_ERR_DECODE is how this header spells it, as for ADPCM), then Error{Unsupported} for the
    // shapes the device decoder leaves to the decoder below (more than 8 channels; a coded width of 0)
    explicit Pcm(const Params &p) : codec_(p.codec), coded_(symaccel_pcm_coded_bytes(p.codec)), native_bytes_(symaccel_pcm_native_bytes(p.codec)) {
        auto unsupported = [](const char *m) { return Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, m); };
        auto decode_error = [](const char *m) { return Error(Error::Kind::IoError, SYMACCEL_ERR_DECODE, m); };
        if (coded_ == 0) throw unsupported("pcm: invalid codec");                                   // lib.rs:222-224
        if (!p.sample_rate) throw unsupported("pcm: sample rate is required");                      // lib.rs:226-229
        if (!p.channels) throw unsupported("pcm: channels or channel_layout is required");          // lib.rs:239-241
        if (*p.channels < 1) throw unsupported("pcm: number of channels cannot be 0");              // lib.rs:233-235
        nch_ = *p.channels;
        const bool implicit = codec_ >= SYMACCEL_PCM_F32LE;  // the float and log codecs (lib.rs:292-303)
        const std::uint32_t width = coded_ == 8 ? 64 : (implicit ? (coded_ == 4 ? 32 : 16) : 8 * (std::uint32_t)coded_);  // lib.rs:248-262
        if (p.bits_per_coded_sample && *p.bits_per_coded_sample > width) throw decode_error("pcm: bits per coded sample greater-than sample format");  // :266-270
        if (p.bits_per_sample) {
            if (*p.bits_per_sample > width) throw decode_error("pcm: bits per sample is greater-than sample format");  // :274-277
            if (p.bits_per_coded_sample && *p.bits_per_coded_sample > *p.bits_per_sample)
                throw decode_error("pcm: bits per coded sample greater-than bits per sample");  // :280-284
        }
        const std::uint32_t decoded_width = p.bits_per_sample.value_or(width), coded_width = p.bits_per_coded_sample.value_or(decoded_width);  // :287-288
        if (implicit) {
            if (decoded_width != width) throw decode_error("pcm: unexpected bits per sample");        // :295-297
            if (coded_width != width) throw decode_error("pcm: unexpected bits per coded sample");    // :298-300
        }
        shift_ = decoded_width - coded_width;  // :307
        if (nch_ > 8 || (!implicit && shift_ == width)) throw unsupported("pcm: a shape the device decoder refuses");
    }
    static constexpr int kBatchKind = SYMACCEL_BATCH_PCM_DECODE;
    static constexpr bool kBlockInterleave = true;  // (a format leaves the kernel as [packet][frame][channel])
    void set_output_format(SampleFormat f) { native_ = f == SampleFormat::Native; }
    int batch_param() const { return codec_ | (int)(nch_ << 8) | (int)(shift_ << 16); }
    std::size_t batch_chains(std::size_t k) const { return k; }
    std::size_t batch_units(std::size_t) const { return next_units_; }
    std::size_t native_bytes() const { return native_bytes_; }
    std::uint32_t shift() const { return shift_; }
    std::size_t frames_of(const Packet &p) const { return p.data.size() / (coded_ * nch_); }  // lib.rs:320
    // the batch about to be submitted: its slot holds `units` frames per packet
    void prepare(const std::vector<Packet> &batch) {
        next_units_ = 0;
        for (const Packet &p : batch) next_units_ = std::max(next_units_, frames_of(p));
    }
    void fill_slot(const std::vector<Packet> &batch, const symaccel_batch_slot &slot) {
        next_frames_.assign(batch.size(), 0);
        place(batch, static_cast<std::uint8_t *>(slot.input[0]), next_units_, next_frames_);
    }
    void take_state(const symaccel_batch_slot &) {
        frames_.swap(next_frames_);
        units_ = next_units_;
    }
    std::size_t channels() const { return nch_; }
    std::size_t packet_frames(std::size_t i) const { return frames_[i]; }
    // native: BYTES in front of packet i's channel c in [packet][channel][units]; a format: the samples in front of the packet, all channels
    std::size_t plane_offset(std::size_t c, std::size_t i, std::size_t) const {
        return native_ ? (i * nch_ + c) * units_ * native_bytes_ : i * units_ * nch_;
    }
    void decode_batch(Context &ctx, const std::vector<Packet> &batch, std::vector<std::uint8_t> &pcm) {
        prepare(batch);
        units_ = next_units_;
        frames_.assign(batch.size(), 0);
        rows_.resize(batch.size() * units_ * coded_ * nch_);
        place(batch, rows_.data(), units_, frames_);
        pcm.assign(batch.size() * nch_ * units_ * native_bytes_, 0);
        if (batch.empty() || units_ == 0) return;
        ctx.pcm_decode(rows_.data(), units_ * coded_ * nch_, batch.size(), codec_, nch_, shift_, units_, pcm.data(), SampleFormat::Native);
    }

private:
    // every packet's whole frames into its row of `units` frames, zero bytes behind them
    void place(const std::vector<Packet> &batch, std::uint8_t *rows, std::size_t units, std::vector<std::size_t> &frames) const {
        const std::size_t fb = coded_ * nch_, pitch = units * fb;
        for (std::size_t i = 0; i < batch.size(); ++i) {
            frames[i] = frames_of(batch[i]);
            std::copy_n(batch[i].data.data(), frames[i] * fb, rows + i * pitch);
            std::fill(rows + i * pitch + frames[i] * fb, rows + (i + 1) * pitch, 0);
        }
    }
    int codec_;
    std::size_t coded_, native_bytes_, nch_ = 0;
    std::uint32_t shift_ = 0;
    std::size_t units_ = 0, next_units_ = 0;  // frames every packet of the current / the submitted batch occupies
    bool native_ = true;
    std::vector<std::size_t> frames_, next_frames_;
    std::vector<std::uint8_t> rows_;
};

// CodecRegistry (symphonia-core/src/codecs/registry.rs:220-341).  The reference's registry maps a codec id to a factory that is handed
// (params, options) and NOTHING ELSE -- `RegisterableAudioDecoder::try_registry_new` (registry.rs:34-44) -- so a decoder it builds cannot
// be told about its siblings: the factories here find the process-wide batcher themselves (`Batcher::shared()`), exactly as the Rust shim's
// `try_registry_new` goes through `Pool::shared()` (decoder.rs, aac.rs).  `register_audio_decoder` = registry.rs:252-269,
// `make_audio_decoder` = registry.rs:330-341 (`Error::Unsupported("core (codec): unsupported codec")` for an id nobody registered).
// The packet source stands where the reference has the FormatReader the decoder is read behind (LookaheadReader in the shim).
struct AudioDecoderOptions {  // codecs/audio.rs:208-222 (`verify`) + the look-ahead of this backend (the shim's DEFAULT_LOOKAHEAD = 256)
    bool verify = false;
    std::size_t lookahead = 256;
};

class CodecRegistry {
public:
    template <class Codec>
    void register_audio_decoder() {
        ids_.insert(std::type_index(typeid(Codec)));
    }
    template <class Codec>
    bool is_registered() const {
        return ids_.count(std::type_index(typeid(Codec))) != 0;
    }
    template <class Codec>
    std::unique_ptr<LookaheadDecoder<Codec>> make_audio_decoder(const typename Codec::Params &params, const AudioDecoderOptions &opts,
                                                                typename LookaheadDecoder<Codec>::Peek peek) const {
        require<Codec>();
        auto dec = std::make_unique<LookaheadDecoder<Codec>>(Batcher::shared(), params, opts.lookahead, std::move(peek));
        if (opts.verify) dec->set_verify(true);  // (a codec that does not verify decodes as ever: the reference's verify nothing either)
        return dec;
    }
    // (zero-copy parse, for the codecs with kDirect)
    template <class Codec>
    std::unique_ptr<LookaheadDecoder<Codec>> make_audio_decoder(const typename Codec::Params &params, const AudioDecoderOptions &opts,
                                                                typename LookaheadDecoder<Codec>::Direct direct) const {
        require<Codec>();
        return std::make_unique<LookaheadDecoder<Codec>>(Batcher::shared(), params, opts.lookahead, std::move(direct));
    }

private:
    template <class Codec>
    void require() const {
        if (!is_registered<Codec>()) throw Error(Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED, "core (codec): unsupported codec");
    }
    std::set<std::type_index> ids_;
};

// symphonia::default::register_enabled_codecs' counterpart for this backend (the shim's `register()`): every codec of the twin
inline void register_enabled_codecs(CodecRegistry &registry) {
    registry.register_audio_decoder<AacLc>();
    registry.register_audio_decoder<AacLcCoded>();
    registry.register_audio_decoder<Mp3>();
    registry.register_audio_decoder<Mp3Huffman>();
    registry.register_audio_decoder<Vorbis>();
    registry.register_audio_decoder<Flac>();
}
// ... and ADPCM, entered by a call of its own (the shim's `adpcm::register`): the list above is the one the shim's `register()` has
inline void register_adpcm(CodecRegistry &registry) { registry.register_audio_decoder<Adpcm>(); }
// ... and PCM / G.711 (the twenty CODEC_ID_PCM_* of symphonia-codec-pcm), likewise
inline void register_pcm(CodecRegistry &registry) { registry.register_audio_decoder<Pcm>(); }
// ... and MPEG Layer I / II (CODEC_ID_MP1 / CODEC_ID_MP2), likewise
inline void register_mpa12(CodecRegistry &registry) { registry.register_audio_decoder<Mpa12>(); }

}  // namespace codecs

}  // namespace symphonia_accel

#endif  // SYMACCEL_HPP
