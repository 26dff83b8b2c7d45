// codecs::Pcm behind LookaheadDecoder, register_pcm and Context::pcm_decode (include/symaccel.hpp) against tests/golden/pcm_decode.npz: the
// reference's own PcmDecoder::try_new + decode_ref on packet sequences of all twenty codecs (tests/test_pcm_decode_cpp.py writes the
// fixture's packets, planes and recorded try_new refusals into the flat file named by argv[1]).  Per fixture case: the direct call on
// every packet; a decoder made by CodecRegistry after register_pcm (on the shared batcher), look-ahead 3 over the eight packets -- batches
// of packets of different lengths, the empty ones included -- and again after reset(); a decoder without a batcher, look-ahead 4; a
// decoder that delivers S16 bytes, against the direct call's S16.  The constructor's refusals carry the reference's variants in the
// reference's order (DecodeError is Kind::IoError with the status SYMACCEL_ERR_DECODE, as for ADPCM); the shapes the device leaves to the
// decoder below are Unsupported; an unregistered codec is Unsupported.  Two decoders of one shape share launches (the batcher's statistics).
// Built against the real library on the GPU box and against the CPU emulation build elsewhere.
#include <cstdio>
#include <cstring>
#include <fstream>
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

struct Case {
    uint32_t codec, channels, shift, bps, bpcs, max_frames, native;
    std::vector<Pcm::Packet> packets;
    std::vector<uint32_t> frames;
    std::vector<std::vector<uint8_t>> planes;  // [packet]: channels x frames x native bytes
    Pcm::Params params() const {
        Pcm::Params p;
        p.codec = (int)codec;
        p.sample_rate = 8000;
        p.channels = channels;
        if (bps) p.bits_per_sample = bps;
        if (bpcs) p.bits_per_coded_sample = bpcs;
        p.max_frames_per_packet = max_frames;
        return p;
    }
};
struct Refusal {
    uint32_t codec, rate, channels, bps, bpcs, kind;  // kind: 1 = Unsupported, 2 = DecodeError
};

static uint32_t rd32(std::ifstream &f) {
    uint32_t v = 0;
    f.read(reinterpret_cast<char *>(&v), 4);
    return v;
}

static bool load(const char *path, std::vector<Case> *cases, std::vector<Refusal> *refusals) {
    std::ifstream f(path, std::ios::binary);
    if (!f || rd32(f) != 0x464d4350u) return false;  // "PCMF"
    const uint32_t n = rd32(f);
    for (uint32_t i = 0; i < n; ++i) {
        Case c;
        c.codec = rd32(f), c.channels = rd32(f), c.shift = rd32(f), c.bps = rd32(f), c.bpcs = rd32(f), c.max_frames = rd32(f), c.native = rd32(f);
        const uint32_t np = rd32(f);
        for (uint32_t j = 0; j < np; ++j) {
            Pcm::Packet p;
            p.ts = j + 1;
            p.data.resize(rd32(f));
            c.frames.push_back(rd32(f));
            f.read(reinterpret_cast<char *>(p.data.data()), (std::streamsize)p.data.size());
            std::vector<uint8_t> pl((size_t)c.channels * c.frames.back() * c.native);
            f.read(reinterpret_cast<char *>(pl.data()), (std::streamsize)pl.size());
            c.packets.push_back(std::move(p));
            c.planes.push_back(std::move(pl));
        }
        cases->push_back(std::move(c));
    }
    const uint32_t nr = rd32(f);
    for (uint32_t i = 0; i < nr; ++i) {
        Refusal r;
        r.codec = rd32(f), r.rate = rd32(f), r.channels = rd32(f), r.bps = rd32(f), r.bpcs = rd32(f), r.kind = rd32(f);
        refusals->push_back(r);
    }
    return (bool)f;
}

static bool same_planes(const Case &c, size_t i, const AudioBufferRefT<uint8_t> &got) {
    if (got.frames != c.frames[i] || got.planes.size() != c.channels) return false;
    const size_t pb = (size_t)c.frames[i] * c.native;
    for (size_t ch = 0; ch < c.channels; ++ch)
        if (pb && std::memcmp(got.planes[ch], c.planes[i].data() + ch * pb, pb) != 0) return false;
    return true;
}

static void run_case(Context &ctx, const CodecRegistry &registry, const Case &c, size_t index) {
    const Pcm::Params params = c.params();
    const std::vector<Pcm::Packet> &track = c.packets;
    // the direct call, packet by packet
    for (size_t i = 0; i < track.size(); ++i) {
        std::vector<uint8_t> got(c.planes[i].size() + 8, 0xEE);
        ctx.pcm_decode(track[i].data.data(), track[i].data.size(), 1, (int)c.codec, c.channels, c.shift, c.frames[i], got.data());
        EXPECT(std::memcmp(got.data(), c.planes[i].data(), c.planes[i].size()) == 0 && got[c.planes[i].size()] == 0xEE, "case %zu packet %zu: the direct call differs from the fixture",
               index, i);
    }
    size_t cur_a = 1, cur_b = 1, cur_c = 1;
    auto peek_a = [&]() -> std::optional<Pcm::Packet> { return cur_a < track.size() ? std::optional<Pcm::Packet>(track[cur_a++]) : std::nullopt; };
    auto peek_b = [&]() -> std::optional<Pcm::Packet> { return cur_b < track.size() ? std::optional<Pcm::Packet>(track[cur_b++]) : std::nullopt; };
    auto peek_c = [&]() -> std::optional<Pcm::Packet> { return cur_c < track.size() ? std::optional<Pcm::Packet>(track[cur_c++]) : std::nullopt; };
    AudioDecoderOptions opts;
    opts.lookahead = 3;
    auto pooled = registry.make_audio_decoder<Pcm>(params, opts, peek_a);
    auto bytes = registry.make_audio_decoder<Pcm>(params, opts, peek_b);
    bytes->set_output(SampleFormat::S16);
    LookaheadDecoder<Pcm> own(ctx, params, 4, peek_c);
    for (int round = 0; round < 2; ++round) {
        cur_a = cur_b = cur_c = 1;
        for (size_t i = 0; i < track.size(); ++i) {
            EXPECT(same_planes(c, i, pooled->decode(track[i])), "case %zu round %d packet %zu: the pooled decoder differs from the fixture", index, round, i);
            EXPECT(same_planes(c, i, own.decode(track[i])), "case %zu round %d packet %zu: the decoder without a batcher differs from the fixture", index, round, i);
            bytes->decode(track[i]);
            const DecodedBytes &d = bytes->last_decoded_bytes();
            std::vector<uint8_t> want((size_t)c.frames[i] * c.channels * 2);
            ctx.pcm_decode(track[i].data.data(), track[i].data.size(), 1, (int)c.codec, c.channels, c.shift, c.frames[i], want.data(), SampleFormat::S16);
            EXPECT(d.frames == c.frames[i] && d.channels == c.channels && d.bytes == want.size() && (want.empty() || (d.data && std::memcmp(d.data, want.data(), want.size()) == 0)),
                   "case %zu round %d packet %zu: the S16 bytes differ from the direct call", index, round, i);
        }
        EXPECT(pooled->batches_run() == (size_t)(round + 1) * ((track.size() + 2) / 3), "case %zu: %zu batches", index, pooled->batches_run());
        pooled->reset();
        bytes->reset();
        own.reset();
    }
}

template <class F>
static int outcome(F f) {  // 0 = fine, 1 = Unsupported, 2 = DecodeError, 3 = anything else
    try {
        f();
        return 0;
    } catch (const Error &e) {
        if (e.kind == Error::Kind::Unsupported && e.status == SYMACCEL_ERR_UNSUPPORTED) return 1;
        return e.kind == Error::Kind::IoError && e.status == SYMACCEL_ERR_DECODE ? 2 : 3;
    } catch (const std::exception &) {
        return 3;
    }
}

static void constructor_errors(const std::vector<Refusal> &refusals) {
    for (const Refusal &r : refusals) {
        Pcm::Params p;
        p.codec = (int)r.codec;  // (0: a codec that is not PCM)
        if (r.rate) p.sample_rate = r.rate;
        if (r.channels) p.channels = r.channels;
        if (r.bps) p.bits_per_sample = r.bps;
        if (r.bpcs) p.bits_per_coded_sample = r.bpcs;
        EXPECT(outcome([&] { Pcm c(p); }) == (int)r.kind, "codec %u rate %u ch %u bps %u bpcs %u: not the reference's variant %u", r.codec, r.rate, r.channels, r.bps, r.bpcs, r.kind);
    }
    // the order of the checks (lib.rs:222-241): the codec before the rate before the channels before the widths
    Pcm::Params p;
    p.codec = 0;
    p.bits_per_sample = 99;
    EXPECT(outcome([&] { Pcm c(p); }) == 1, "invalid codec comes first");
    p.codec = SYMACCEL_PCM_S16LE;
    EXPECT(outcome([&] { Pcm c(p); }) == 1, "then the sample rate");
    p.sample_rate = 8000;
    EXPECT(outcome([&] { Pcm c(p); }) == 1, "then the channels");
    p.channels = 0;
    EXPECT(outcome([&] { Pcm c(p); }) == 1, "no channels");
    p.channels = 2;
    EXPECT(outcome([&] { Pcm c(p); }) == 2, "then the widths");
    p.bits_per_sample = 16;
    p.bits_per_coded_sample = 12;
    EXPECT(outcome([&] { Pcm c(p); EXPECT(c.shift() == 4 && c.native_bytes() == 2, "shift"); }) == 0, "a legal shift");
    // left to the decoder below: more than 8 channels; a coded width of 0
    p.channels = 9;
    EXPECT(outcome([&] { Pcm c(p); }) == 1, "nine channels");
    p.channels = 2;
    p.bits_per_coded_sample.reset();
    p.bits_per_sample = 0;
    EXPECT(outcome([&] { Pcm c(p); }) == 0, "bits per sample 0 with no coded width: shift 0");
}

static void sharing(const CodecRegistry &registry, const Case &c) {
    // two decoders of one shape, each with its whole track in the look-ahead: their batches meet in one launch
    symaccel_batcher_stats before, after;
    symaccel_batcher_get_stats(Batcher::shared().raw(), &before);
    size_t cur_a = 1, cur_b = 1;
    const std::vector<Pcm::Packet> &track = c.packets;
    auto peek_a = [&]() -> std::optional<Pcm::Packet> { return cur_a < track.size() ? std::optional<Pcm::Packet>(track[cur_a++]) : std::nullopt; };
    auto peek_b = [&]() -> std::optional<Pcm::Packet> { return cur_b < track.size() ? std::optional<Pcm::Packet>(track[cur_b++]) : std::nullopt; };
    AudioDecoderOptions opts;
    opts.lookahead = 16;
    auto a = registry.make_audio_decoder<Pcm>(c.params(), opts, peek_a);
    auto b = registry.make_audio_decoder<Pcm>(c.params(), opts, peek_b);
    for (size_t i = 0; i < track.size(); ++i) {
        EXPECT(same_planes(c, i, a->decode(track[i])), "sharing: decoder a packet %zu", i);
        EXPECT(same_planes(c, i, b->decode(track[i])), "sharing: decoder b packet %zu", i);
    }
    symaccel_batcher_get_stats(Batcher::shared().raw(), &after);
    EXPECT(after.submissions - before.submissions == 2 && after.failed_tickets == before.failed_tickets, "sharing: %llu submissions",
           (unsigned long long)(after.submissions - before.submissions));
    EXPECT(after.launches - before.launches <= 2, "sharing: %llu launches", (unsigned long long)(after.launches - before.launches));
}

int main(int argc, char **argv) {
    std::vector<Case> cases;
    std::vector<Refusal> refusals;
    if (argc < 2 || !load(argv[1], &cases, &refusals) || cases.size() < 20 || refusals.size() < 10) {
        std::printf("FAIL: the fixture file (argv[1]) is missing or short\n");
        return 1;
    }
    try {
        Context ctx(0);
        CodecRegistry none, registry;
        EXPECT(outcome([&] { none.make_audio_decoder<Pcm>(cases[0].params(), AudioDecoderOptions{}, LookaheadDecoder<Pcm>::Peek()); }) == 1, "an unregistered codec");
        register_enabled_codecs(none);
        EXPECT(!none.is_registered<Pcm>(), "register_enabled_codecs keeps its list");
        register_pcm(registry);
        for (size_t i = 0; i < cases.size(); ++i) run_case(ctx, registry, cases[i], i);
        constructor_errors(refusals);
        sharing(registry, cases[1]);
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
