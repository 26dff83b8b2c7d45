// codecs::Flac verifying its stream (the STREAMINFO MD5, symphonia-bundle-flac validate.rs:25-75, decoder.rs:231-234, 272-308) behind
// LookaheadDecoder, built through CodecRegistry::make_audio_decoder with AudioDecoderOptions::verify.  The streams, the PCM every packet
// must give and the digests (hashlib's: of the whole stream, of its first six packets, of the stream without packets 6 and 7) come from
// tests/test_flac_verify_cpp.py in a file: nothing expected here is computed by the library under test.  A two-channel stream takes the
// finishing form of the batcher's kind (param 0x300 | shift), a three-channel one the plain verify form (0x200).  Built against the
// real library on the GPU box and against the CPU emulation build elsewhere.
#include <array>
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

using Digest = std::array<uint8_t, 16>;

struct Stream {
    Flac::Params params;
    std::vector<Flac::Packet> packets;
    std::vector<std::vector<int32_t>> pcm;  // [packet][channel][blocksize]
    Digest whole, first6, without67;
};

static std::vector<Stream> load(const char *path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open the case file");
    auto u32 = [&] {
        uint32_t v = 0;
        in.read(reinterpret_cast<char *>(&v), 4);
        return v;
    };
    std::vector<Stream> streams(u32());
    for (Stream &s : streams) {
        const size_t nch = u32();
        s.params.channels = nch;
        s.params.bits_per_sample = u32();
        s.params.max_blocksize = u32();
        s.packets.resize(u32());
        s.pcm.resize(s.packets.size());
        for (Digest *d : {&s.whole, &s.first6, &s.without67}) in.read(reinterpret_cast<char *>(d->data()), 16);
        for (size_t i = 0; i < s.packets.size(); ++i) {
            Flac::Packet &p = s.packets[i];
            p.ts = 5000 + i;
            p.blocksize = u32();
            p.pair_mode = (uint8_t)u32();
            p.words.resize(nch * p.blocksize);
            p.desc.resize(nch);
            p.coeffs.resize(nch * 32);
            s.pcm[i].resize(nch * p.blocksize);
            in.read(reinterpret_cast<char *>(p.words.data()), (std::streamsize)(p.words.size() * 4));
            in.read(reinterpret_cast<char *>(p.desc.data()), (std::streamsize)(nch * sizeof(symaccel_flac_desc)));
            in.read(reinterpret_cast<char *>(p.coeffs.data()), (std::streamsize)(p.coeffs.size() * 4));
            in.read(reinterpret_cast<char *>(s.pcm[i].data()), (std::streamsize)(s.pcm[i].size() * 4));
        }
        if (!in) throw std::runtime_error("the case file is short");
    }
    return streams;
}

// a decoder from the registry over `track`, the demuxer's cursor in `cur`
struct Track {
    const std::vector<Flac::Packet> &track;
    size_t cur = 1;
    std::unique_ptr<LookaheadDecoder<Flac>> dec;
    Track(const CodecRegistry &registry, const Flac::Params &params, const std::vector<Flac::Packet> &t, bool verify = true) : track(t) {
        AudioDecoderOptions opts;
        opts.verify = verify;
        opts.lookahead = 4;
        dec = registry.make_audio_decoder<Flac>(params, opts, [this]() -> std::optional<Flac::Packet> {
            return cur < track.size() ? std::optional<Flac::Packet>(track[cur++]) : std::nullopt;
        });
    }
    bool decode(const Stream &s, size_t i, bool compare = true) {
        if (cur <= i) cur = i + 1;  // (the demuxer is past the packet being decoded)
        const AudioBufferRefS32 &got = dec->decode(track[i]);
        const size_t n = track[i].blocksize;
        bool same = got.frames == n && got.planes.size() == s.params.channels;
        for (size_t c = 0; compare && same && c < s.params.channels; ++c) same = std::memcmp(got.planes[c], s.pcm[i].data() + c * n, n * 4) == 0;
        return same;
    }
};

static void run(const CodecRegistry &registry, const Stream &s, const char *what) {
    const size_t n = s.packets.size();
    Flac::Params with = s.params;
    with.expected_md5 = s.whole;
    {  // the whole stream across batch boundaries: every packet exact, the digest is STREAMINFO's
        Track t(registry, with, s.packets);
        EXPECT(!t.dec->finalize().verify_ok.has_value() || !*t.dec->finalize().verify_ok, "%s: nothing decoded yet is not the stream's digest", what);
        for (size_t i = 0; i < n; ++i) EXPECT(t.decode(s, i), "%s packet %zu: the PCM differs", what, i);
        EXPECT(t.dec->batches_run() == 4, "%s: %zu batches", what, t.dec->batches_run());
        const FinalizeResult r = t.dec->finalize();
        EXPECT(r.verify_ok.has_value() && *r.verify_ok, "%s: finalize() must be Some(true)", what);
    }
    {  // one residual bit flipped: Some(false), the other packets keep their PCM
        std::vector<Flac::Packet> bad = s.packets;
        bad[5].words[0] ^= 1;
        Track t(registry, with, bad);
        for (size_t i = 0; i < n; ++i) EXPECT(t.decode(s, i, i != 5), "%s packet %zu beside the damaged one", what, i);
        const FinalizeResult r = t.dec->finalize();
        EXPECT(r.verify_ok.has_value() && !*r.verify_ok, "%s: a flipped bit must give Some(false)", what);
    }
    {  // no digest in STREAMINFO: nothing to say (decoder.rs:302-304); verification off: likewise
        Track t(registry, s.params, s.packets), off(registry, with, s.packets, false);
        for (size_t i = 0; i < n; ++i) EXPECT(t.decode(s, i) && off.decode(s, i), "%s packet %zu", what, i);
        EXPECT(!t.dec->finalize().verify_ok.has_value() && !off.dec->finalize().verify_ok.has_value(), "%s: no verdict without a digest / without verify", what);
    }
    {  // the checkpoint rule: after 6 of the 13 packets the digest is that of 6 frames, though two batches were computed
        Flac::Params six = s.params;
        six.expected_md5 = s.first6;
        Track t(registry, six, s.packets);
        for (size_t i = 0; i < 6; ++i) EXPECT(t.decode(s, i), "%s packet %zu", what, i);
        EXPECT(t.dec->finalize().verify_ok.value_or(false), "%s: finalize() after six packets is the digest of six frames", what);
        // ... and reset() leaves the validator alone (decoder.rs:254-256): decoding on completes the stream's digest
        t.dec->reset();
        t.cur = 7;
        for (size_t i = 6; i < n; ++i) EXPECT(t.decode(s, i), "%s packet %zu after reset()", what, i);
        EXPECT(!t.dec->finalize().verify_ok.value_or(true), "%s: thirteen frames are not the digest of six", what);
        Track u(registry, with, s.packets);
        for (size_t i = 0; i < 6; ++i) u.decode(s, i);
        u.dec->reset();
        u.cur = 7;
        for (size_t i = 6; i < n; ++i) u.decode(s, i);
        EXPECT(u.dec->finalize().verify_ok.value_or(false), "%s: reset() in mid-stream keeps the hash going", what);
    }
    {  // two packets skipped without reset(): the replay hashes nothing, the skipped frames are not in the digest
        Flac::Params skip = s.params;
        skip.expected_md5 = s.without67;
        Track t(registry, skip, s.packets);
        for (size_t i = 0; i < n; ++i) {
            if (i == 6 || i == 7) continue;
            if (i == 8) t.cur = 9;  // (the demuxer moved with the caller)
            EXPECT(t.decode(s, i), "%s packet %zu around the skip", what, i);
        }
        EXPECT(t.dec->finalize().verify_ok.value_or(false), "%s: the digest after a skip is that of the packets handed out", what);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::printf("usage: flac_verify_test <case file>\n");
        return 2;
    }
    try {
        const std::vector<Stream> streams = load(argv[1]);
        CodecRegistry registry;
        register_enabled_codecs(registry);
        symaccel_batcher_stats s0{}, s1{};
        symaccel_batcher_get_stats(Batcher::shared().raw(), &s0);
        run(registry, streams[0], "two channels (0x300)");
        run(registry, streams[1], "three channels (0x200)");
        symaccel_batcher_get_stats(Batcher::shared().raw(), &s1);
        EXPECT(s1.failed_tickets == s0.failed_tickets && s1.submissions > s0.submissions, "the shared batcher ran the verify forms");
        // two decoders share launches: their look-ahead batches, submitted ahead, go to the device together
        for (const Stream &s : streams) {
            Flac::Params with = s.params;
            with.expected_md5 = s.whole;
            Track a(registry, with, s.packets), b(registry, with, s.packets);
            symaccel_batcher_stats before{}, after{};
            symaccel_batcher_get_stats(Batcher::shared().raw(), &before);
            for (size_t i = 0; i < s.packets.size(); ++i) EXPECT(a.decode(s, i) && b.decode(s, i), "shared launch, packet %zu", i);
            symaccel_batcher_get_stats(Batcher::shared().raw(), &after);
            EXPECT(after.submissions - before.submissions == 8 && after.launches - before.launches < 8, "two decoders: %llu launches for 8 submissions",
                   (unsigned long long)(after.launches - before.launches));
            EXPECT(a.dec->finalize().verify_ok.value_or(false) && b.dec->finalize().verify_ok.value_or(false), "both streams verify");
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
