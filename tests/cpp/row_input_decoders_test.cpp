// codecs::Flac behind LookaheadDecoder with a width per row (Batcher::InputMode::Rows, SYMACCEL_IN_FMT_ROWS): six streams made by
// tests/test_row_input_decoders.py -- per packet the words, descriptors and coefficients the front end would hand over, the PCM the oracle
// restores from them, and hashlib's MD5 of the stream -- are decoded, look-ahead 4 over 13 packets, in the mode SYMACCEL_NARROW_INPUT names.
//   0: 16 bit, 2 channels, every word fits int16_t        1: the same with ONE 17-bit side warm-up in packet 5      2: 16 bit, 3 channels
//   3: 24 bit, 2 channels, every word fits 24 bits        4: the same with ONE 25-bit side warm-up in packet 5      5: 24 bit, 1 channel, 4097
// In every mode the PCM equals the file's (the wide path's).  Mode 1 sends the batch with the 17-bit word wide, as it always did; mode 2
// sends that batch with one row at 3 bytes and the rest at 2.  The rows per width are counted here from the packets' words, and the bytes
// of plane 0 handed to the batcher equal the sum the widths give.  Verifying, finalize() is Some(true).
//   row_input_decoders_test <case file> 0|1|2      (the mode; SYMACCEL_NARROW_INPUT is set to it, or unset for 0, and the Batcher must have read it)
// Built against the real library on the GPU box and against the CPU emulation build elsewhere.
#include <algorithm>
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
    std::array<size_t, 3> rows{{0, 0, 0}};  // the rows (subframes) whose narrowest width is 2, 3, 4 bytes a word
    std::vector<int> packet_width;          // the widest row of every packet
    size_t n_rows() const { return rows[0] + rows[1] + rows[2]; }
    // the whole-batch rule over the batches of packets 0..3, 4..7, 8..11 and 12: a batch goes narrow when every word of it fits int16_t
    size_t narrow_batches() const {
        size_t n = 0;
        for (size_t b = 0; b < packets.size(); b += 4) n += narrow_batch(b) ? 1 : 0;
        return n;
    }
    size_t narrow_batch_rows() const {
        size_t n = 0;
        for (size_t b = 0; b < packets.size(); b += 4) n += narrow_batch(b) ? (std::min(b + 4, packets.size()) - b) * params.channels : 0;
        return n;
    }
    bool narrow_batch(size_t b) const {
        for (size_t i = b; i < std::min(b + 4, packets.size()); ++i)
            if (packet_width[i] > 2) return false;
        return true;
    }
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
            for (size_t c = 0; c < nch; ++c) {
                int w = 2;
                for (size_t k = 0; k < p.blocksize; ++k) {
                    const int64_t v = p.words[c * p.blocksize + k];
                    if (v < -8388608 || v > 8388607) w = 4;
                    else if ((v < -32768 || v > 32767) && w < 3) w = 3;
                }
                s.rows[(size_t)w - 2] += 1;
                if (c == 0) s.packet_width.push_back(w);
                else s.packet_width.back() = std::max(s.packet_width.back(), w);
            }
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

int main(int argc, char **argv) {
    if (argc < 3) {
        std::printf("usage: row_input_decoders_test <case file> 0|1|2\n");
        return 2;
    }
    const int mode = std::atoi(argv[2]);
    try {
        const std::vector<Stream> streams = load(argv[1]);
        EXPECT(streams.size() == 6, "six streams");
        EXPECT(streams[0].rows == (std::array<size_t, 3>{{26, 0, 0}}) && streams[1].rows == (std::array<size_t, 3>{{25, 1, 0}}), "the 16-bit streams' rows");
        EXPECT(streams[0].narrow_batches() == 4 && streams[1].narrow_batches() == 3 && streams[1].narrow_batch_rows() == 18 && streams[3].narrow_batches() == 0,
               "the whole-batch rule on the streams as written");
        EXPECT(streams[3].rows[2] == 0 && streams[3].rows[1] > 0 && streams[4].rows[2] == 1 && streams[5].rows[2] == 0, "the 24-bit streams' rows");
        Context ctx(0);
        Batcher batcher(ctx, 0);
        EXPECT((int)batcher.input_mode() == mode, "the Batcher reads SYMACCEL_NARROW_INPUT when it is made (default: wide): %d", (int)batcher.input_mode());
        EXPECT(batcher.narrow_input() == (mode == 1), "narrow_input() is the whole-batch rule alone");
        for (const bool verify : {false, true}) {
            // every stream through the one batcher, interleaved packet by packet: their batches share launches
            std::vector<std::unique_ptr<Track>> tracks;
            for (const Stream &s : streams) tracks.emplace_back(new Track(batcher, s, verify));
            for (size_t i = 0; i < streams[0].packets.size(); ++i)
                for (auto &t : tracks) EXPECT(t->decode(i), "mode %d%s, stream %zu, packet %zu: the PCM differs", mode, verify ? ", verifying" : "", (size_t)(&t->s - streams.data()), i);
            for (size_t k = 0; k < tracks.size(); ++k) {
                const Stream &s = streams[k];
                const LookaheadDecoder<Flac> &d = *tracks[k]->dec;
                const size_t nb = d.narrow_batches(), wb = d.wide_batches(), row = s.params.max_blocksize;
                const std::array<size_t, 3> sent = d.rows_sent();
                if (verify) EXPECT(tracks[k]->dec->finalize().verify_ok.value_or(false), "mode %d, stream %zu: finalize() must be Some(true)", mode, k);
                if (mode == 2) {  // a width per row: what the words need, no more; neither kind of whole batch is counted
                    EXPECT(sent == s.rows, "stream %zu: %zu + %zu + %zu rows sent, %zu + %zu + %zu expected", k, sent[0], sent[1], sent[2], s.rows[0], s.rows[1], s.rows[2]);
                    EXPECT(nb == 0 && wb == 0, "stream %zu: %zu narrow and %zu wide batches in the per-row mode", k, nb, wb);
                    EXPECT(d.plane0_bytes() == row * (2 * s.rows[0] + 3 * s.rows[1] + 4 * s.rows[2]), "stream %zu: %zu bytes of plane 0", k, d.plane0_bytes());
                    continue;
                }
                EXPECT(sent == (std::array<size_t, 3>{{0, 0, 0}}), "stream %zu: no row has a width of its own in mode %d", k, mode);
                EXPECT(nb + wb == 4, "stream %zu: %zu narrow and %zu wide batches", k, nb, wb);
                // mode 1: the batch that holds packet 5 of stream 1 goes wide whole, for its one 17-bit word
                const size_t want_nb = mode == 0 ? 0 : s.narrow_batches();
                EXPECT(nb == want_nb, "stream %zu: %zu narrow batches, %zu expected", k, nb, want_nb);
                const size_t narrow_rows = mode == 0 ? 0 : s.narrow_batch_rows();
                EXPECT(d.plane0_bytes() == row * (2 * narrow_rows + 4 * (s.n_rows() - narrow_rows)), "stream %zu: %zu bytes of plane 0", k, d.plane0_bytes());
            }
        }
        {  // the setters: a decoder follows what the batcher says when it attaches
            batcher.set_input_mode(Batcher::InputMode::Rows);
            Track t(batcher, streams[1], false);
            for (size_t i = 0; i < streams[1].packets.size(); ++i) EXPECT(t.decode(i), "set_input_mode(Rows), packet %zu", i);
            EXPECT(t.dec->rows_sent() == streams[1].rows, "set_input_mode(Rows) is what a decoder that attaches afterwards follows");
            batcher.set_narrow_input(true);
            EXPECT(batcher.input_mode() == Batcher::InputMode::NarrowBatches, "set_narrow_input(true) is the whole-batch rule");
            batcher.set_narrow_input(false);
            EXPECT(batcher.input_mode() == Batcher::InputMode::Wide, "set_narrow_input(false) is wide");
            batcher.set_input_mode(static_cast<Batcher::InputMode>(mode));
        }
        {  // reset() in mid-stream
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
