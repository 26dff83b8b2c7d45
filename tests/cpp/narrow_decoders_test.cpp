// codecs::Flac behind LookaheadDecoder sending its batches up as int16_t (symaccel_batcher_reserve_io) when every word of a batch fits:
// four 16-bit streams made by tests/test_narrow_decoders.py -- per packet the words, descriptors and coefficients the front end would hand
// over, the PCM the oracle restores from them, and hashlib's MD5 of the stream -- are decoded, look-ahead 4 over 13 packets, through a
// batcher that narrows and through one that does not.  The PCM of both equals the file's; the narrowing decoders send NO batch wide (the
// inputs are built to fit: a silent fall-back cannot hide) and the others none narrow; in the fifth stream, which has ONE 17-bit side
// warm-up in packet 5, exactly the batch that holds that packet goes wide; verifying, finalize() is still Some(true).
//   narrow_decoders_test <case file> on|off      on: SYMACCEL_NARROW_INPUT=1 is set in the environment, and the Batcher must have read it
// Built against the real library on the GPU box and against the CPU emulation build elsewhere.
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
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

struct Stream {
    Flac::Params params;
    std::vector<Flac::Packet> packets;
    std::vector<std::vector<int32_t>> pcm;  // [packet][channel][blocksize]
    std::array<uint8_t, 16> whole;
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
        in.read(reinterpret_cast<char *>(s.whole.data()), 16);
        for (size_t i = 0; i < s.packets.size(); ++i) {
            Flac::Packet &p = s.packets[i];
            p.ts = 7000 + i;
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

struct Track {
    const Stream &s;
    size_t cur = 1;
    std::unique_ptr<LookaheadDecoder<Flac>> dec;
    Track(Batcher &batcher, const Stream &stream, bool verify) : s(stream) {
        Flac::Params p = s.params;
        p.verify = verify;
        if (verify) p.expected_md5 = s.whole;
        dec.reset(new LookaheadDecoder<Flac>(batcher, p, 4, [this]() -> std::optional<Flac::Packet> {
            return cur < s.packets.size() ? std::optional<Flac::Packet>(s.packets[cur++]) : std::nullopt;
        }));
    }
    bool decode(size_t i) {
        if (cur <= i) cur = i + 1;
        const AudioBufferRefS32 &got = dec->decode(s.packets[i]);
        const size_t n = s.packets[i].blocksize;
        bool same = got.frames == n && got.planes.size() == s.params.channels;
        for (size_t c = 0; same && c < s.params.channels; ++c) same = std::memcmp(got.planes[c], s.pcm[i].data() + c * n, n * 4) == 0;
        return same;
    }
};

// every stream through `batcher`, interleaved packet by packet (their batches share launches); the decoders are returned for their counters
static std::vector<std::unique_ptr<Track>> decode_all(Batcher &batcher, const std::vector<Stream> &streams, size_t first, size_t count, bool verify, const char *what) {
    std::vector<std::unique_ptr<Track>> tracks;
    for (size_t k = first; k < first + count; ++k) tracks.emplace_back(new Track(batcher, streams[k], verify));
    for (size_t i = 0; i < streams[first].packets.size(); ++i)
        for (auto &t : tracks) EXPECT(t->decode(i), "%s, stream of %zu channels, packet %zu: the PCM differs", what, t->s.params.channels, i);
    return tracks;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        std::printf("usage: narrow_decoders_test <case file> on|off\n");
        return 2;
    }
    const bool on = std::string(argv[2]) == "on";
    try {
        const std::vector<Stream> streams = load(argv[1]);  // 0..3 fit; 4 has one 17-bit side warm-up in packet 5
        Context ctx(0);
        Batcher batcher(ctx, 0);
        EXPECT(batcher.narrow_input() == on, "the Batcher reads SYMACCEL_NARROW_INPUT when it is made (default: off)");
        for (const bool verify : {false, true}) {
            auto tracks = decode_all(batcher, streams, 0, 4, verify, verify ? "verifying" : "plain");
            for (auto &t : tracks) {
                const size_t nb = t->dec->narrow_batches(), wb = t->dec->wide_batches();
                EXPECT(nb + wb == 4 && (on ? wb == 0 && nb > 0 : nb == 0), "%zu narrow and %zu wide batches", nb, wb);
                if (verify) EXPECT(t->dec->finalize().verify_ok.value_or(false), "finalize() must be Some(true)");
            }
        }
        {  // the same batcher told otherwise: the PCM is the same, and the choice follows
            batcher.set_narrow_input(!on);
            auto tracks = decode_all(batcher, streams, 0, 4, false, "set_narrow_input(the other way)");
            for (auto &t : tracks) EXPECT(on ? t->dec->narrow_batches() == 0 : t->dec->wide_batches() == 0, "set_narrow_input() is what a decoder that attaches afterwards follows");
            batcher.set_narrow_input(on);
        }
        for (const bool verify : {false, true}) {  // packets 4..7 are the second batch: it alone goes wide
            auto tracks = decode_all(batcher, streams, 4, 1, verify, "one 17-bit warm-up");
            const size_t nb = tracks[0]->dec->narrow_batches(), wb = tracks[0]->dec->wide_batches();
            EXPECT(on ? (nb == 3 && wb == 1) : (nb == 0 && wb == 4), "one 17-bit warm-up: %zu narrow and %zu wide batches", nb, wb);
            if (verify) EXPECT(tracks[0]->dec->finalize().verify_ok.value_or(false), "one 17-bit warm-up: finalize() must be Some(true)");
        }
        {  // reset() in mid-stream: the batch after it is judged on its own
            Track t(batcher, streams[4], false);
            for (size_t i = 0; i < 3; ++i) EXPECT(t.decode(i), "before reset(), packet %zu", i);
            t.dec->reset();
            t.cur = 4;
            for (size_t i = 3; i < streams[4].packets.size(); ++i) EXPECT(t.decode(i), "after reset(), packet %zu", i);
        }
        const symaccel_batcher_stats st = batcher.stats();
        EXPECT(st.failed_tickets == 0 && st.submissions > 0, "no ticket failed");
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
