// codecs::Adpcm behind LookaheadDecoder, Context::adpcm_decode and the registry entry (include/symaccel.hpp) against a scalar host
// decoder written after symphonia-codec-adpcm (codec_ms.rs:89-136, common_ima.rs:38-48, codec_ima_wav.rs:27-65, codec_ima_qt.rs:14-47):
// packet bytes -> the trait's planes [channel][block * fpb + frame] for the three codecs, mono and stereo, several blocks per packet and
// a short last packet, across look-ahead batch boundaries and after reset(); the same track delivered as S16 bytes; rejected blocks, short
// packets and refused shapes with the reference's error class (the C++ Error has no DecodeError kind: an IMA WAV step index out of range is
// Kind::IoError carrying the status SYMACCEL_ERR_DECODE), each failing ALONE inside a look-ahead batch.  Built against the real library on the GPU box and against the CPU
// emulation build elsewhere (tests/test_adpcm_cpp.py).
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

// ---- the host decoder ------------------------------------------------------------------------------------------------------------
static const int kStep[89] = {7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173,
                              190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878,
                              2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899,
                              15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};
static const int kIndex[16] = {-1, -1, -1, -1, 2, 4, 6, 8, -1, -1, -1, -1, 2, 4, 6, 8};
static const int kAdapt[16] = {230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230};
static const int kC1[7] = {256, 512, 0, 192, 240, 460, 392}, kC2[7] = {0, -256, 0, 64, 0, -208, -232};

static int32_t clamp16(int64_t v) { return (int32_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }
static int32_t wrap(int64_t v) { return (int32_t)(uint32_t)(uint64_t)v; }
static int32_t shl16(int32_t v) { return (int32_t)((uint32_t)v << 16); }
static int32_t rd16(const uint8_t *p) { return (int16_t)(uint16_t)(p[0] | p[1] << 8); }

struct Ima {
    int32_t pred, idx;
    int32_t nibble(unsigned n) {
        const int32_t diff = ((2 * (int32_t)(n & 7) + 1) * kStep[idx]) >> 3;
        pred = clamp16((n & 8) ? pred - diff : pred + diff);
        idx = std::min(88, std::max(0, idx + kIndex[n]));
        return shl16(pred);
    }
};
struct Ms {
    int32_t c1, c2, delta, s1, s2;
    int32_t nibble(unsigned n) {
        const int32_t sn = (n & 8) ? (int32_t)n - 16 : (int32_t)n;
        const int32_t pred = wrap((int64_t)((s1 * c1 + s2 * c2) / 256) + wrap((int64_t)sn * delta));
        s2 = s1;
        s1 = clamp16(pred);
        delta = std::max(16, wrap((int64_t)kAdapt[n] * delta) / 256);
        return shl16(s1);
    }
};

// one block -> out[c][0 .. fpb); 0, or the status of the rejected preamble
static int host_block(int codec, size_t nch, size_t fpb, const uint8_t *b, int32_t *const out[2]) {
    if (codec == SYMACCEL_ADPCM_MS) {
        Ms st[2];
        for (size_t c = 0; c < nch; ++c) {
            if (b[c] > 6) return 1;
            st[c] = Ms{kC1[b[c]], kC2[b[c]], rd16(b + nch + 2 * c), rd16(b + 3 * nch + 2 * c), rd16(b + 5 * nch + 2 * c)};
            out[c][0] = shl16(st[c].s2);
            out[c][1] = shl16(st[c].s1);
        }
        const uint8_t *d = b + 7 * nch;
        if (nch == 1)
            for (size_t k = 1; k < fpb / 2; ++k, ++d) out[0][2 * k] = st[0].nibble(*d >> 4), out[0][2 * k + 1] = st[0].nibble(*d & 15);
        else
            for (size_t f = 2; f < fpb; ++f, ++d) out[0][f] = st[0].nibble(*d >> 4), out[1][f] = st[1].nibble(*d & 15);
    } else if (codec == SYMACCEL_ADPCM_IMA_WAV) {
        Ima st[2];
        for (size_t c = 0; c < nch; ++c) {
            if (b[4 * c + 2] > 88) return 2;
            st[c] = Ima{rd16(b + 4 * c), b[4 * c + 2]};
            out[c][0] = shl16(st[c].pred);
        }
        const uint8_t *d = b + 4 * nch;
        if (nch == 1)
            for (size_t k = 0; k < (fpb - 1) / 2; ++k, ++d) out[0][1 + 2 * k] = st[0].nibble(*d & 15), out[0][2 + 2 * k] = st[0].nibble(*d >> 4);
        else
            for (size_t k = 0; k < fpb - 1; ++k, ++d) {
                const size_t c = (k / 4) & 1, at = 1 + (k / 8) * 8 + (k % 4) * 2;
                out[c][at] = st[c].nibble(*d & 15);
                out[c][at + 1] = st[c].nibble(*d >> 4);
            }
    } else {
        for (size_t c = 0; c < nch; ++c) {
            const unsigned h = (unsigned)b[34 * c] << 8 | b[34 * c + 1];
            Ima st{(int16_t)(uint16_t)(h & 0xff80), (int32_t)std::min(88u, h & 0x7fu)};
            for (size_t k = 0; k < 32; ++k) out[c][2 * k] = st.nibble(b[34 * c + 2 + k] & 15), out[c][2 * k + 1] = st.nibble(b[34 * c + 2 + k] >> 4);
        }
    }
    return 0;
}

// a packet -> planes[c][block * fpb + frame]
static std::vector<std::vector<int32_t>> host_packet(const Adpcm::Params &p, const Adpcm::Packet &pkt) {
    const size_t n = pkt.block_dur / p.frames_per_block, bytes = symaccel_adpcm_block_bytes(p.codec, p.channels, p.frames_per_block);
    std::vector<std::vector<int32_t>> planes(p.channels, std::vector<int32_t>(n * p.frames_per_block));
    for (size_t j = 0; j < n; ++j) {
        int32_t *out[2] = {planes[0].data() + j * p.frames_per_block, planes[p.channels - 1].data() + j * p.frames_per_block};
        host_block(p.codec, p.channels, p.frames_per_block, pkt.data.data() + j * bytes, out);
    }
    return planes;
}

static std::vector<Adpcm::Packet> make_track(const Adpcm::Params &p, size_t packets, unsigned seed) {
    std::mt19937 rng(seed);
    const size_t bytes = symaccel_adpcm_block_bytes(p.codec, p.channels, p.frames_per_block), bpp = p.max_frames_per_packet / p.frames_per_block;
    std::vector<Adpcm::Packet> track(packets);
    for (size_t i = 0; i < packets; ++i) {
        const size_t n = i + 1 == packets ? std::max<size_t>(1, bpp - 1) : bpp;  // a short last packet
        track[i].ts = 1000 + i;
        track[i].block_dur = n * p.frames_per_block + (i % 2 ? p.frames_per_block / 2 : 0);  // (a remainder below one block is dropped, lib.rs:131)
        track[i].data.resize(n * bytes + (i % 3));                                            // (trailing bytes are ignored)
        for (uint8_t &v : track[i].data) v = (uint8_t)rng();
        for (size_t j = 0; j < n; ++j)
            for (size_t c = 0; c < p.channels; ++c) {
                if (p.codec == SYMACCEL_ADPCM_MS) track[i].data[j * bytes + c] %= 7;
                if (p.codec == SYMACCEL_ADPCM_IMA_WAV) track[i].data[j * bytes + 4 * c + 2] %= 89;
            }
    }
    return track;
}

static void run(Batcher &b, const Adpcm::Params &params, size_t lookahead, const char *what) {
    const std::vector<Adpcm::Packet> track = make_track(params, 11, (unsigned)(params.codec * 10 + params.channels));
    size_t cur_a = 0, cur_b = 0, cur_c = 0;
    auto peek_a = [&]() -> std::optional<Adpcm::Packet> { return cur_a < track.size() ? std::optional<Adpcm::Packet>(track[cur_a++]) : std::nullopt; };
    auto peek_b = [&]() -> std::optional<Adpcm::Packet> { return cur_b < track.size() ? std::optional<Adpcm::Packet>(track[cur_b++]) : std::nullopt; };
    auto peek_c = [&]() -> std::optional<Adpcm::Packet> { return cur_c < track.size() ? std::optional<Adpcm::Packet>(track[cur_c++]) : std::nullopt; };
    LookaheadDecoder<Adpcm> planar(b, params, lookahead, peek_a), bytes(b, params, lookahead, peek_b), own(b.context(), params, lookahead, peek_c);
    (void)own;
    bytes.set_output(SampleFormat::S16);
    bool threw = false;
    try {
        bytes.set_output(SampleFormat::S16, false);
    } catch (const Error &e) {
        threw = e.kind == Error::Kind::Unsupported;
    }
    EXPECT(threw, "%s: a planar format is refused", what);
    for (int round = 0; round < 2; ++round) {
        cur_a = cur_b = 1;
        for (size_t i = 0; i < track.size(); ++i) {
            const std::vector<std::vector<int32_t>> want = host_packet(params, track[i]);
            const AudioBufferRefS32 &got = planar.decode(track[i]);
            EXPECT(got.frames == want[0].size() && got.planes.size() == params.channels, "%s packet %zu: %zu frames", what, i, got.frames);
            bool same = got.frames == want[0].size();
            for (size_t c = 0; same && c < params.channels; ++c) same = std::memcmp(got.planes[c], want[c].data(), got.frames * 4) == 0;
            EXPECT(same, "%s packet %zu: the planes differ from the host decoder", what, i);
            bytes.decode(track[i]);
            const DecodedBytes &d = bytes.last_decoded_bytes();
            EXPECT(d.frames == want[0].size() && d.channels == params.channels && d.bytes == d.frames * d.channels * 2 && d.data, "%s packet %zu: bytes shape", what, i);
            bool same16 = d.data != nullptr && d.frames == want[0].size();
            for (size_t f = 0; same16 && f < d.frames; ++f)
                for (size_t c = 0; c < params.channels; ++c) {
                    int16_t v;
                    std::memcpy(&v, d.data + (f * params.channels + c) * 2, 2);
                    if (v != (int16_t)(want[c][f] >> 16)) same16 = false;
                }
            EXPECT(same16, "%s packet %zu: the S16 bytes differ", what, i);
        }
        EXPECT(planar.batches_run() >= (size_t)(round + 1) * 3, "%s: %zu batches", what, planar.batches_run());
        planar.reset();
        bytes.reset();
    }
    // without a batcher: the context's own call
    cur_c = 1;
    for (size_t i = 0; i < 5; ++i) {
        const std::vector<std::vector<int32_t>> want = host_packet(params, track[i]);
        const AudioBufferRefS32 &got = own.decode(track[i]);
        bool same = got.frames == want[0].size();
        for (size_t c = 0; same && c < params.channels; ++c) same = std::memcmp(got.planes[c], want[c].data(), got.frames * 4) == 0;
        EXPECT(same, "%s packet %zu: the planes of the decoder without a batcher differ", what, i);
    }
}

template <class F>
static bool throws_error(F f, Error::Kind kind, int status) {
    try {
        f();
    } catch (const Error &e) {
        return e.kind == kind && (status == 0 || e.status == status);
    } catch (...) {
    }
    return false;
}

int main() {
    try {
        Context ctx(0);
        {
            Batcher b(ctx);
            run(b, Adpcm::Params{SYMACCEL_ADPCM_MS, 2, 35, 3 * 35}, 4, "MS stereo");
            run(b, Adpcm::Params{SYMACCEL_ADPCM_MS, 1, 132, 2 * 132}, 4, "MS mono");
            run(b, Adpcm::Params{SYMACCEL_ADPCM_IMA_WAV, 1, 41, 4 * 41}, 3, "IMA WAV mono");
            run(b, Adpcm::Params{SYMACCEL_ADPCM_IMA_WAV, 2, 73, 2 * 73}, 4, "IMA WAV stereo");
            run(b, Adpcm::Params{SYMACCEL_ADPCM_IMA_QT, 2, 64, 5 * 64}, 4, "IMA QT stereo");
            run(b, Adpcm::Params{SYMACCEL_ADPCM_IMA_QT, 1, 64, 64}, 4, "IMA QT mono");

            // rejected blocks and short packets: the reference's error class, and the decoder goes on with the next packet
            for (int codec : {SYMACCEL_ADPCM_MS, SYMACCEL_ADPCM_IMA_WAV}) {
                const Adpcm::Params p{codec, 2, codec == SYMACCEL_ADPCM_MS ? (size_t)35 : (size_t)73, 2 * (codec == SYMACCEL_ADPCM_MS ? (size_t)35 : (size_t)73)};
                std::vector<Adpcm::Packet> track = make_track(p, 3, 99);
                const size_t bytes = symaccel_adpcm_block_bytes(p.codec, 2, p.frames_per_block);
                track[0].data[bytes + (codec == SYMACCEL_ADPCM_MS ? 1 : 6)] = 200;  // the second block of the first packet
                for (int with_batcher = 0; with_batcher < 2; ++with_batcher) {
                    LookaheadDecoder<Adpcm> with(b, p, 1, nullptr), without(ctx, p, 1, nullptr);
                    LookaheadDecoder<Adpcm> &dec = with_batcher ? with : without;
                    EXPECT(throws_error([&] { dec.decode(track[0]); }, codec == SYMACCEL_ADPCM_MS ? Error::Kind::Unsupported : Error::Kind::IoError,
                                        codec == SYMACCEL_ADPCM_MS ? SYMACCEL_ERR_UNSUPPORTED : SYMACCEL_ERR_DECODE),
                           "codec %d (batcher %d): a rejected block", codec, with_batcher);
                    EXPECT(dec.last_decoded().frames == 0, "the buffer is cleared after an error");
                    const std::vector<std::vector<int32_t>> want = host_packet(p, track[1]);
                    const AudioBufferRefS32 &got = dec.decode(track[1]);
                    EXPECT(got.frames == want[0].size() && std::memcmp(got.planes[1], want[1].data(), got.frames * 4) == 0, "codec %d: the packet after the bad one", codec);
                    Adpcm::Packet cut = track[2];
                    cut.data.resize(bytes - 1);
                    EXPECT(throws_error([&] { dec.decode(cut); }, Error::Kind::IoError, 0), "codec %d: a packet shorter than its blocks", codec);
                }
            }
        }
        // A packet fails ALONE inside a look-ahead batch: lookahead 4 over six packets, a rejected block in the second block of packet 2, packet 4
        // one byte short -- their neighbours in the same batches keep their PCM, and each error comes when its own packet is decoded
        {
            Batcher b(ctx);
            for (int codec : {SYMACCEL_ADPCM_MS, SYMACCEL_ADPCM_IMA_WAV}) {
                const size_t fpb = codec == SYMACCEL_ADPCM_MS ? 35 : 73;
                const Adpcm::Params p{codec, 2, fpb, 2 * fpb};
                std::vector<Adpcm::Packet> track = make_track(p, 6, 123);
                const size_t bytes = symaccel_adpcm_block_bytes(p.codec, 2, p.frames_per_block);
                track[2].data[bytes + (codec == SYMACCEL_ADPCM_MS ? 1 : 6)] = 200;
                track[4].data.resize(2 * bytes - 1);
                for (int with_batcher = 0; with_batcher < 2; ++with_batcher) {
                    size_t cur = 1;
                    auto peek = [&]() -> std::optional<Adpcm::Packet> { return cur < track.size() ? std::optional<Adpcm::Packet>(track[cur++]) : std::nullopt; };
                    LookaheadDecoder<Adpcm> with(b, p, 4, peek), without(ctx, p, 4, peek);
                    LookaheadDecoder<Adpcm> &dec = with_batcher ? with : without;
                    for (size_t i = 0; i < track.size(); ++i) {
                        if (cur <= i) cur = i + 1;  // (the demuxer is past the packet being decoded)
                        if (i == 2) {
                            EXPECT(throws_error([&] { dec.decode(track[i]); }, codec == SYMACCEL_ADPCM_MS ? Error::Kind::Unsupported : Error::Kind::IoError,
                                                codec == SYMACCEL_ADPCM_MS ? SYMACCEL_ERR_UNSUPPORTED : SYMACCEL_ERR_DECODE),
                                   "codec %d (batcher %d): packet 2 carries the rejected block", codec, with_batcher);
                            EXPECT(dec.last_decoded().frames == 0, "the buffer is cleared after an error");
                        } else if (i == 4) {
                            EXPECT(throws_error([&] { dec.decode(track[i]); }, Error::Kind::IoError, 0), "codec %d (batcher %d): packet 4 is short", codec, with_batcher);
                        } else {
                            const std::vector<std::vector<int32_t>> want = host_packet(p, track[i]);
                            bool ok = false;
                            try {
                                const AudioBufferRefS32 &got = dec.decode(track[i]);
                                ok = got.frames == want[0].size() && std::memcmp(got.planes[0], want[0].data(), got.frames * 4) == 0 &&
                                     std::memcmp(got.planes[1], want[1].data(), got.frames * 4) == 0;
                            } catch (const std::exception &e) {
                                std::printf("packet %zu threw: %s\n", i, e.what());
                            }
                            EXPECT(ok, "codec %d (batcher %d): packet %zu beside the bad ones keeps its PCM", codec, with_batcher, i);
                        }
                    }
                    EXPECT(dec.batches_run() == 2, "codec %d (batcher %d): %zu batches for six packets at look-ahead 4", codec, with_batcher, dec.batches_run());
                }
            }
        }
        // refused shapes go to the decoder below
        for (const Adpcm::Params &p : {Adpcm::Params{SYMACCEL_ADPCM_MS, 1, 3, 30}, Adpcm::Params{SYMACCEL_ADPCM_MS, 2, 1, 30}, Adpcm::Params{SYMACCEL_ADPCM_IMA_WAV, 1, 40, 400},
                                       Adpcm::Params{SYMACCEL_ADPCM_IMA_WAV, 2, 10, 400}, Adpcm::Params{SYMACCEL_ADPCM_IMA_QT, 1, 32, 64}, Adpcm::Params{SYMACCEL_ADPCM_MS, 3, 20, 40},
                                       Adpcm::Params{SYMACCEL_ADPCM_MS, 2, 20, 0}, Adpcm::Params{7, 2, 20, 40}})
            EXPECT(throws_error([&] { Adpcm a(p); }, Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED), "codec %d channels %zu fpb %zu is refused", p.codec, p.channels, p.frames_per_block);
        // Context::adpcm_decode: the host form, every block of a packet at once, with a status array
        {
            const Adpcm::Params p{SYMACCEL_ADPCM_IMA_WAV, 2, 17, 4 * 17};
            std::vector<Adpcm::Packet> track = make_track(p, 2, 5);
            track[0].data[24 + 2] = 89;  // the second block
            std::vector<int32_t> pcm(4 * 2 * 17, 1);
            std::vector<int16_t> s16(4 * 2 * 17, 1);
            std::vector<uint8_t> status(4, 9);
            ctx.adpcm_decode(track[0].data.data(), 24, 4, p.codec, 2, 17, pcm.data(), SampleFormat::Native, status.data());
            ctx.adpcm_decode(track[0].data.data(), 24, 4, p.codec, 2, 17, s16.data(), SampleFormat::S16);
            EXPECT(status[0] == 0 && status[1] == 2 && status[2] == 0 && status[3] == 0, "status %d %d %d %d", status[0], status[1], status[2], status[3]);
            for (size_t j = 0; j < 4; ++j) {
                std::vector<int32_t> l(17, 0), r(17, 0);
                int32_t *out[2] = {l.data(), r.data()};
                host_block(p.codec, 2, 17, track[0].data.data() + 24 * j, out);
                bool same = std::memcmp(pcm.data() + (2 * j) * 17, l.data(), 68) == 0 && std::memcmp(pcm.data() + (2 * j + 1) * 17, r.data(), 68) == 0;
                for (size_t f = 0; f < 17; ++f) same = same && s16[(j * 17 + f) * 2] == (int16_t)(l[f] >> 16) && s16[(j * 17 + f) * 2 + 1] == (int16_t)(r[f] >> 16);
                EXPECT(same, "adpcm_decode block %zu", j);
            }
            EXPECT(throws_error([&] { ctx.adpcm_decode(track[0].data.data(), 24, 4, p.codec, 2, 18, pcm.data()); }, Error::Kind::Unsupported, SYMACCEL_ERR_UNSUPPORTED), "a refused shape");
        }
        // the registry: ADPCM is entered by its own call, and the decoder it makes sits on the shared batcher
        {
            CodecRegistry registry;
            register_enabled_codecs(registry);
            EXPECT(!registry.is_registered<Adpcm>(), "register_enabled_codecs keeps its list");
            const Adpcm::Params p{SYMACCEL_ADPCM_IMA_QT, 2, 64, 2 * 64};
            EXPECT(throws_error([&] { registry.make_audio_decoder<Adpcm>(p, AudioDecoderOptions{}, LookaheadDecoder<Adpcm>::Peek()); }, Error::Kind::Unsupported, 0), "unregistered");
            register_adpcm(registry);
            EXPECT(registry.is_registered<Adpcm>() && registry.is_registered<Flac>(), "register_adpcm");
            const std::vector<Adpcm::Packet> track = make_track(p, 4, 77);
            size_t cur = 1;
            AudioDecoderOptions opts;
            opts.lookahead = 2;
            auto dec = registry.make_audio_decoder<Adpcm>(p, opts, [&]() -> std::optional<Adpcm::Packet> { return cur < track.size() ? std::optional<Adpcm::Packet>(track[cur++]) : std::nullopt; });
            symaccel_batcher_stats before{}, after{};
            symaccel_batcher_get_stats(Batcher::shared().raw(), &before);
            for (size_t i = 0; i < track.size(); ++i) {
                const std::vector<std::vector<int32_t>> want = host_packet(p, track[i]);
                const AudioBufferRefS32 &got = dec->decode(track[i]);
                EXPECT(got.frames == want[0].size() && std::memcmp(got.planes[0], want[0].data(), got.frames * 4) == 0 && std::memcmp(got.planes[1], want[1].data(), got.frames * 4) == 0,
                       "registry decoder packet %zu", i);
            }
            symaccel_batcher_get_stats(Batcher::shared().raw(), &after);
            EXPECT(after.submissions - before.submissions == 2 && after.launches > before.launches && after.failed_tickets == before.failed_tickets, "the shared batcher ran the batches");
        }
    } catch (const std::exception &e) {
        std::printf("FAIL: exception: %s\n", e.what());
        return 1;
    }
    if (g_failures) {
        std::printf("%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
