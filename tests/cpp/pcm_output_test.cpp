// LookaheadDecoder::set_output (include/symaccel.hpp): a decoder that delivers S16 interleaved bytes, converted in the batcher's scatter,
// against the SAME track through a decoder that returns the planar buffer, converted on the host with the reference's FromSample
// arithmetic (audio/conv.rs:602 from f32, :527 from i32) -- packet by packet, across look-ahead batch boundaries and after reset().
// AAC-LC, MP3 and Vorbis (f32 planes) and two-channel FLAC (left-justified i32 planes) share one batcher.  Built against the real
// library on the GPU box and against the CPU emulation build elsewhere (tests/test_pcm_output_cpp.py).
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "symaccel.hpp"

using namespace symphonia_accel;
using namespace symphonia_accel::codecs;

static int g_failures = 0;
#define EXPECT(cond, ...)                                    \
    do {                                                     \
        if (!(cond)) {                                       \
            ++g_failures;                                    \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
        }                                                    \
    } while (0)

// conv.rs:602 with clamp_f32 (util.rs:258-266); `as i16` truncates and saturates
static int16_t s16_from_f32(float s) {
    float c = s > 1.0f ? 1.0f : s;
    c = c < -1.0f ? -1.0f : c;
    const float v = c * 32768.0f;
    if (v != v) return 0;
    return v >= 32767.0f ? 32767 : (v <= -32768.0f ? -32768 : (int16_t)v);
}
static int16_t s16_from_i32(int32_t s) { return (int16_t)(s >> 16); }  // conv.rs:527
static int16_t to_s16(float s) { return s16_from_f32(s); }
static int16_t to_s16(int32_t s) { return s16_from_i32(s); }

// one packet: the planar buffer on the host against the bytes of the converting decoder
template <class S>
static bool packet_matches(const AudioBufferRefT<S> &planar, const DecodedBytes &got, bool interleaved, const char *what, size_t i) {
    const size_t nch = planar.planes.size(), nf = planar.frames;
    EXPECT(got.frames == nf && got.channels == nch && got.format == SampleFormat::S16, "%s packet %zu: shape %zu x %zu", what, i, got.frames, got.channels);
    if (got.frames != nf || got.channels != nch) return false;
    if (nf == 0) return true;
    EXPECT(got.data != nullptr, "%s packet %zu: no data", what, i);
    if (!got.data) return false;
    EXPECT(got.bytes == (interleaved ? nf * nch * 2 : nf * 2), "%s packet %zu: %zu bytes", what, i, got.bytes);
    for (size_t f = 0; f < nf; ++f)
        for (size_t c = 0; c < nch; ++c) {
            int16_t v;
            std::memcpy(&v, interleaved ? got.data + (f * nch + c) * 2 : got.data + c * got.plane_stride + f * 2, 2);
            if (v != to_s16(planar.planes[c][f])) {
                EXPECT(false, "%s packet %zu frame %zu channel %zu: %d, the host conversion gives %d", what, i, f, c, (int)v, (int)to_s16(planar.planes[c][f]));
                return false;
            }
        }
    return true;
}

// the same track through two decoders on one batcher; `visit` = the packet indices in order, -1 = reset() of both
template <class Codec>
static void run(Batcher &b, const typename Codec::Params &params, const std::vector<typename Codec::Packet> &track, size_t lookahead, const std::vector<int> &visit,
                bool interleaved, const char *what) {
    size_t cur_a = 0, cur_b = 0;
    auto peek_a = [&]() -> std::optional<typename Codec::Packet> { return cur_a < track.size() ? std::optional<typename Codec::Packet>(track[cur_a++]) : std::nullopt; };
    auto peek_b = [&]() -> std::optional<typename Codec::Packet> { return cur_b < track.size() ? std::optional<typename Codec::Packet>(track[cur_b++]) : std::nullopt; };
    LookaheadDecoder<Codec> planar(b, params, lookahead, peek_a), bytes(b, params, lookahead, peek_b);
    bytes.set_output(SampleFormat::S16, interleaved);
    EXPECT(bytes.last_decoded_bytes().data == nullptr && bytes.last_decoded_bytes().frames == 0, "%s: bytes before the first decode", what);
    size_t packets = 0;
    for (int at : visit) {
        if (at < 0) {
            planar.reset();
            bytes.reset();
            EXPECT(bytes.last_decoded_bytes().frames == 0 && bytes.last_decoded().is_empty(), "%s: reset() must clear the buffer", what);
            continue;
        }
        const size_t i = (size_t)at;
        if (cur_a <= i) cur_a = i + 1;
        if (cur_b <= i) cur_b = i + 1;
        const auto &want = planar.decode(track[i]);
        const auto &ref = bytes.decode(track[i]);
        EXPECT(ref.frames == want.frames, "%s packet %zu: decode() must keep returning the frame count (%zu vs %zu)", what, i, ref.frames, want.frames);
        for (const auto *p : ref.planes) EXPECT(p == nullptr, "%s packet %zu: the planar ref of a converting decoder holds no planes", what, i);
        if (!packet_matches(want, bytes.last_decoded_bytes(), interleaved, what, i)) return;
        ++packets;
    }
    EXPECT(bytes.batches_run() > 1 && bytes.batches_run() < packets, "%s: %zu batches for %zu packets", what, bytes.batches_run(), packets);
    bool threw = false;
    try {
        bytes.set_output(SampleFormat::Native);  // in the middle of a batch
    } catch (const std::logic_error &) {
        threw = true;
    }
    EXPECT(threw, "%s: set_output between batches only", what);
}

static std::vector<int> visits(int n, int seek_at, int seek_to) {
    std::vector<int> v;
    for (int i = 0; i < seek_at; ++i) v.push_back(i);
    v.push_back(-1);
    for (int i = seek_to; i < n; ++i) v.push_back(i);
    return v;
}

static std::vector<AacLc::Packet> aac_track(size_t n, size_t nch, unsigned seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.0f, 400.0f);  // (loud: a share of the samples leaves [-1, 1] and saturates)
    std::vector<AacLc::Packet> t(n);
    int cur = 0, prev_shape = 1;
    for (size_t i = 0; i < n; ++i) {
        cur = (cur == 0 || cur == 3) ? ((rng() % 4 == 0) ? 1 : 0) : ((rng() % 2) ? 2 : 3);
        const int shape = (int)(rng() % 2);
        t[i].ts = 1000 + 1024 * i;
        t[i].coeffs.resize(nch * 1024);
        for (auto &v : t[i].coeffs) v = nd(rng);
        t[i].side.assign(nch, SYMACCEL_AAC_SIDE((unsigned)cur, (unsigned)shape, (unsigned)prev_shape));
        prev_shape = shape;
    }
    return t;
}

static std::vector<Mp3::Packet> mp3_track(size_t n, size_t nch, size_t ngr, unsigned seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.0f, 0.3f);
    std::vector<Mp3::Packet> t(n);
    for (size_t i = 0; i < n; ++i) {
        t[i].ts = 5000 + 1152 * i;
        t[i].xr.resize(ngr * nch * 576);
        t[i].side.resize(ngr * nch);
        for (size_t gr = 0; gr < ngr; ++gr) {
            const unsigned rz = 2 * (unsigned)(rng() % 289);
            for (size_t c = 0; c < nch; ++c) {
                float *x = t[i].xr.data() + (gr * nch + c) * 576;
                for (unsigned k = 0; k < 576; ++k) x[k] = k < rz ? nd(rng) : 0.0f;
                t[i].side[gr * nch + c] = symaccel_mp3_side{0, 0, (uint16_t)rz};
            }
        }
    }
    return t;
}

static std::vector<Vorbis::Packet> vorbis_track(size_t n, size_t nch, int e0, int e1, unsigned seed) {
    const size_t bs[2] = {(size_t)1 << e0, (size_t)1 << e1};
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.0f, 0.6f);
    std::vector<Vorbis::Packet> t(n);
    for (size_t i = 0; i < n; ++i) {
        t[i].ts = 9000 + 7 * i;
        t[i].long_block = rng() % 3 != 0;
        t[i].spectra.resize(nch * bs[t[i].long_block] / 2);
        for (auto &v : t[i].spectra) v = nd(rng);
    }
    return t;
}

static std::vector<Flac::Packet> flac_track(size_t n, size_t nch, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<Flac::Packet> t(n);
    for (size_t i = 0; i < n; ++i) {
        Flac::Packet &p = t[i];
        p.ts = 900 + 4096 * i;
        p.blocksize = i + 1 == n ? 777 : (rng() % 4 == 0 ? 1152 : 4096);
        p.words.resize(nch * p.blocksize);
        p.desc.resize(nch);
        p.coeffs.assign(nch * 32, 0);
        p.pair_mode = (uint8_t)(rng() % 4);
        for (size_t c = 0; c < nch; ++c) {
            const unsigned kind = rng() % 2;  // verbatim or fixed
            p.desc[c] = symaccel_flac_desc{(uint8_t)kind, (uint8_t)(kind ? rng() % 3 : 0), 0, 0};
            for (size_t k = 0; k < p.blocksize; ++k) p.words[c * p.blocksize + k] = (int32_t)(rng() % 801) - 400;
        }
    }
    return t;
}

int main(int argc, char **argv) {
    const bool expect_no_device = argc > 1 && std::strcmp(argv[1], "--expect-no-device") == 0;
    try {
        Context ctx(0);
        if (expect_no_device) {
            std::printf("a context was created although no device was expected\n");
            return 1;
        }
        Batcher batcher(ctx, 0);
        const size_t K = 6;
        run<AacLc>(batcher, AacLc::Params{2}, aac_track(29, 2, 3), K, visits(29, 15, 17), true, "AAC");
        run<AacLc>(batcher, AacLc::Params{2}, aac_track(20, 2, 4), K, visits(20, 9, 9), false, "AAC planar");
        run<Mp3>(batcher, Mp3::Params{2, 2, 1}, mp3_track(25, 2, 2, 5), K, visits(25, 11, 14), true, "MP3");
        run<Vorbis>(batcher, Vorbis::Params{2, 8, 11}, vorbis_track(31, 2, 8, 11, 6), K, visits(31, 14, 19), true, "Vorbis");
        run<Vorbis>(batcher, Vorbis::Params{2, 6, 9}, vorbis_track(22, 2, 6, 9, 7), K, visits(22, 10, 10), false, "Vorbis planar");
        run<Flac>(batcher, Flac::Params{2, 16, 4096}, flac_track(23, 2, 8), K, visits(23, 9, 9), true, "FLAC");
        // what set_output refuses: no batcher under the decoder; a FLAC layout that is finished on the host
        {
            LookaheadDecoder<AacLc> direct(ctx, AacLc::Params{2}, 4, nullptr);
            bool threw = false;
            try {
                direct.set_output(SampleFormat::S16);
            } catch (const std::invalid_argument &) {
                threw = true;
            }
            EXPECT(threw, "set_output without a batcher");
            LookaheadDecoder<Flac> mono(batcher, Flac::Params{1, 16, 4096}, 4, nullptr);
            threw = false;
            try {
                mono.set_output(SampleFormat::S16);
            } catch (const Error &e) {
                threw = e.kind == Error::Kind::Unsupported;
            }
            EXPECT(threw, "set_output on a mono FLAC stream");
        }
        // Context::pcm_convert: the host form
        {
            std::vector<float> planes(2 * 100);
            for (size_t i = 0; i < planes.size(); ++i) planes[i] = (float)i / 150.0f - 0.6f;
            std::vector<int16_t> out(200, 77);
            ctx.pcm_convert(planes.data(), SampleFormat::F32, 100, 1, 2, 100, out.data(), SampleFormat::S16, 400);
            for (size_t f = 0; f < 100; ++f)
                for (size_t c = 0; c < 2; ++c) EXPECT(out[f * 2 + c] == s16_from_f32(planes[c * 100 + f]), "pcm_convert frame %zu channel %zu", f, c);
            EXPECT(sample_bytes(SampleFormat::S24) == 3 && sample_bytes(SampleFormat::Native) == 0, "sample_bytes");
        }
    } catch (const Error &e) {
        if (expect_no_device && e.kind == Error::Kind::IoError) {
            std::printf("no device, as expected: %s\n", e.what());
            return 0;
        }
        std::printf("error: %s\n", e.what());
        return 1;
    }
    if (g_failures) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
