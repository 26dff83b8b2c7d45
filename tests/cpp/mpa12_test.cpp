// codecs::Mpa12 behind LookaheadDecoder, Context::mpa12_decode and the registry entry (include/symaccel.hpp) against a scalar host
// decoder: the dequantisation of layer1/mod.rs:51-60, 156-159 and layer2/mod.rs:198-213, 341-346 written out per sample, followed by
// the CPU oracle's polyphase filterbank (linked as the checker only).  Single-stream scripts -- both layers, mono and stereo, with and
// without a batcher, across look-ahead batch boundaries and a reset() -- and S streams built by the CodecRegistry sharing the process-wide
// batcher.  Built against the real library on the GPU box and against the CPU emulation build elsewhere (tests/test_mpa12_cpp.py).
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "symaccel.hpp"
#include "symoracle.h"

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

static float g_tbl[131];  // SYMACCEL_TABLE_MPA12: FACTOR[16] | SCALEFACTORS[64] | 17 x {c, d, width} (pinned to the reference by tests/test_mpa12.py)

static int32_t sign_extend(uint32_t v, unsigned bits) { return (int32_t)(v << (32 - bits)) >> (32 - bits); }

// one channel-packet: codes[32][nf] + record -> samples[32 * nf]
static void host_dequantize(int layer, const uint16_t *codes, const uint8_t *rec, float *out) {
    const unsigned nf = layer == SYMACCEL_MPA_LAYER1 ? 12 : 36;
    for (unsigned sb = 0; sb < 32; ++sb)
        for (unsigned j = 0; j < nf; ++j) {
            float x = 0.0f;
            if (rec[sb] != 0 && layer == SYMACCEL_MPA_LAYER1) {
                const unsigned bits = rec[sb];
                const uint32_t raw = codes[sb * nf + j] & ((1u << bits) - 1u);
                const int32_t a = sign_extend(raw ^ (1u << (bits - 1)), bits);
                volatile float sample = g_tbl[bits] * (float)(a + 1);
                x = g_tbl[16 + rec[32 + sb]] * sample;
            } else if (rec[sb] != 0) {
                const float *q = g_tbl + 80 + 3 * (rec[sb] - 1);
                const unsigned bits = (unsigned)q[2];
                const uint32_t raw = codes[sb * nf + j] & ((1u << bits) - 1u);
                const int32_t a = sign_extend(raw ^ (1u << (bits - 1)), bits);
                volatile float s = (float)a / (float)(1u << (bits - 1));
                volatile float sum = s + q[1];
                volatile float t = q[0] * sum;
                x = g_tbl[16 + rec[32 + 32 * (j / 12) + sb]] * t;
            }
            out[sb * nf + j] = x;
        }
}

static std::vector<Mpa12::Packet> make_track(const Mpa12::Params &p, size_t n, unsigned seed) {
    std::mt19937 rng(seed);
    const size_t nf = p.layer == SYMACCEL_MPA_LAYER1 ? 12 : 36, rb = symaccel_mpa12_record_bytes(p.layer);
    std::vector<Mpa12::Packet> t(n);
    for (size_t i = 0; i < n; ++i) {
        t[i].ts = 9000 + 32 * nf * i;
        t[i].codes.resize(p.channels * 32 * nf);
        t[i].rec.resize(p.channels * rb);
        for (auto &c : t[i].codes) c = (uint16_t)rng();
        for (size_t c = 0; c < p.channels; ++c)
            for (size_t k = 0; k < rb; ++k) {
                uint8_t v;
                if (k >= 32) v = (uint8_t)(rng() % 64);
                else if (p.layer == SYMACCEL_MPA_LAYER1) v = (uint8_t)(rng() % 4 == 0 ? 0 : 2 + rng() % 14);
                else v = (uint8_t)(rng() % 18);
                t[i].rec[c * rb + k] = v;
            }
    }
    return t;
}

struct HostState {
    std::vector<float> vv;
    std::vector<int> vf;
    explicit HostState(size_t nch) : vv(nch * 1024, 0.0f), vf(nch, 0) {}
    void reset() {
        std::fill(vv.begin(), vv.end(), 0.0f);
        std::fill(vf.begin(), vf.end(), 0);
    }
    // the packet's PCM [channel][32 * nf]
    std::vector<float> decode(const Mpa12::Params &p, const Mpa12::Packet &pk) {
        const size_t nf = p.layer == SYMACCEL_MPA_LAYER1 ? 12 : 36, rb = symaccel_mpa12_record_bytes(p.layer);
        std::vector<float> x(32 * nf), out(p.channels * 32 * nf);
        for (size_t c = 0; c < p.channels; ++c) {
            host_dequantize(p.layer, pk.codes.data() + c * 32 * nf, pk.rec.data() + c * rb, x.data());
            so_mp3_polyphase(vv.data() + c * 1024, &vf[c], (int)nf, x.data(), out.data() + c * 32 * nf);
        }
        return out;
    }
};

static void test_stream(Context &ctx, const Mpa12::Params &p, size_t lookahead, Batcher *batcher) {
    const size_t n = 21, frames = p.layer == SYMACCEL_MPA_LAYER1 ? 384 : 1152;
    const auto track = make_track(p, n, 100 * (unsigned)p.layer + 10 * (unsigned)p.channels + (unsigned)lookahead);
    size_t cursor = 0;
    auto peek = [&]() -> std::optional<Mpa12::Packet> {
        if (cursor >= track.size()) return std::nullopt;
        return track[cursor++];
    };
    std::optional<LookaheadDecoder<Mpa12>> holder;
    if (batcher) holder.emplace(*batcher, p, lookahead, peek);
    else holder.emplace(ctx, p, lookahead, peek);
    LookaheadDecoder<Mpa12> &dec = *holder;
    HostState host(p.channels);
    for (size_t i = 0; i < n; ++i) {
        if (i == 11) {  // seek
            dec.reset();
            host.reset();
            cursor = i;
        }
        if (cursor <= i) cursor = i + 1;
        const AudioBufferRef &buf = dec.decode(track[i]);
        const std::vector<float> want = host.decode(p, track[i]);
        EXPECT(buf.frames == frames, "frames per packet");
        for (size_t c = 0; c < p.channels; ++c)
            EXPECT(std::memcmp(buf.planes[c], want.data() + c * frames, frames * 4) == 0, "layer %d ch %zu K=%zu%s packet %zu channel %zu differs", p.layer, p.channels,
                   lookahead, batcher ? " (batcher)" : "", i, c);
    }
}

// S decoders built by the registry: they sit on the process-wide batcher and share its launches
static void test_registry(size_t n_streams) {
    CodecRegistry registry;
    register_enabled_codecs(registry);
    EXPECT(!registry.is_registered<Mpa12>(), "register_enabled_codecs keeps its list");
    bool refused = false;
    try {
        registry.make_audio_decoder<Mpa12>(Mpa12::Params{}, AudioDecoderOptions{}, LookaheadDecoder<Mpa12>::Peek());
    } catch (const Error &e) {
        refused = e.kind == Error::Kind::Unsupported;
    }
    EXPECT(refused, "an unregistered codec is Unsupported");
    register_mpa12(registry);
    EXPECT(registry.is_registered<Mpa12>() && registry.is_registered<Mp3>(), "register_mpa12");
    const size_t n = 8;
    std::vector<Mpa12::Params> params(n_streams);
    std::vector<std::vector<Mpa12::Packet>> tracks(n_streams);
    std::vector<size_t> cursor(n_streams, 1);
    std::vector<std::unique_ptr<LookaheadDecoder<Mpa12>>> decs;
    std::vector<HostState> hosts;
    AudioDecoderOptions opts;
    opts.lookahead = 4;
    for (size_t s = 0; s < n_streams; ++s) {
        params[s] = Mpa12::Params{s % 3 == 0 ? SYMACCEL_MPA_LAYER1 : SYMACCEL_MPA_LAYER2, 1 + s % 2};
        tracks[s] = make_track(params[s], n, 4000 + (unsigned)s);
        hosts.emplace_back(params[s].channels);
        decs.push_back(registry.make_audio_decoder<Mpa12>(params[s], opts, [&tracks, &cursor, s]() -> std::optional<Mpa12::Packet> {
            return cursor[s] < tracks[s].size() ? std::optional<Mpa12::Packet>(tracks[s][cursor[s]++]) : std::nullopt;
        }));
    }
    symaccel_batcher_stats before{}, after{};
    symaccel_batcher_get_stats(Batcher::shared().raw(), &before);
    for (size_t i = 0; i < n; ++i)
        for (size_t s = 0; s < n_streams; ++s) {
            const size_t frames = params[s].layer == SYMACCEL_MPA_LAYER1 ? 384 : 1152;
            const AudioBufferRef &buf = decs[s]->decode(tracks[s][i]);
            const std::vector<float> want = hosts[s].decode(params[s], tracks[s][i]);
            for (size_t c = 0; c < params[s].channels; ++c)
                EXPECT(buf.frames == frames && std::memcmp(buf.planes[c], want.data() + c * frames, frames * 4) == 0, "registry stream %zu packet %zu channel %zu", s, i, c);
        }
    symaccel_batcher_get_stats(Batcher::shared().raw(), &after);
    EXPECT(after.submissions - before.submissions >= 2 * n_streams && after.launches - before.launches < after.submissions - before.submissions &&
               after.failed_tickets == before.failed_tickets,
           "the decoders share launches: %llu submissions, %llu launches", (unsigned long long)(after.submissions - before.submissions),
           (unsigned long long)(after.launches - before.launches));
}

int main() {
    try {
        EXPECT(symaccel_table_f32(nullptr, SYMACCEL_TABLE_MPA12, g_tbl, 131) == 131, "the table");
        Context ctx(0);
        for (int layer : {SYMACCEL_MPA_LAYER1, SYMACCEL_MPA_LAYER2})
            for (size_t nch : {size_t(1), size_t(2)})
                for (size_t k : {size_t(1), size_t(4), size_t(9)}) test_stream(ctx, Mpa12::Params{layer, nch}, k, nullptr);
        {
            Batcher batcher(ctx);
            for (int layer : {SYMACCEL_MPA_LAYER1, SYMACCEL_MPA_LAYER2})
                for (size_t nch : {size_t(1), size_t(2)})
                    for (size_t k : {size_t(1), size_t(4), size_t(9)}) test_stream(ctx, Mpa12::Params{layer, nch}, k, &batcher);
        }
        {  // Context::mpa12_decode, and a record out of range through the codec
            const Mpa12::Params p{SYMACCEL_MPA_LAYER2, 2};
            auto track = make_track(p, 3, 5);
            Mpa12 codec(p);
            std::vector<float> pcm;
            codec.decode_batch(ctx, track, pcm);
            HostState host(2);
            bool same = true;
            for (size_t i = 0; i < 3; ++i) {
                const std::vector<float> want = host.decode(p, track[i]);
                for (size_t c = 0; c < 2; ++c) same = same && std::memcmp(pcm.data() + (c * 3 + i) * 1152, want.data() + c * 1152, 1152 * 4) == 0;
            }
            EXPECT(same, "decode_batch");
            track[1].rec[3] = 18;
            bool threw = false;
            try {
                Mpa12 again(p);
                again.decode_batch(ctx, track, pcm);
            } catch (const std::invalid_argument &) {
                threw = true;
            }
            EXPECT(threw, "a class above 17 is refused");
            bool unsupported = false;
            try {
                Mpa12 l3(Mpa12::Params{3, 2});
            } catch (const Error &e) {
                unsupported = e.kind == Error::Kind::Unsupported;
            }
            EXPECT(unsupported, "layer 3 is not this codec's");
        }
        test_registry(6);
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
