// codecs::CodecBase (include/symaccel.hpp): what a codec behind LookaheadDecoder must supply, and what it gets when it supplies nothing
// more.  `Toy` below is the smallest codec there is -- the required members and no hook --, decoded through LookaheadDecoder across a
// batch boundary and a skipped packet; every hook's default is then visible from outside.  The codec to copy when a new one is added.
// Built against the real library on the GPU box and against the CPU emulation build elsewhere (tests/test_codec_base_cpp.py).
#include <cstdio>
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

// One channel, 4 frames per packet, decoded on the host: frame f of a packet is value[f] + the last value of the packet before it.
// That carry is the codec's state, with the one-packet memory LookaheadDecoder's replay relies on (the state after a packet depends on
// that packet alone).  kBatchKind 0: never through a Batcher, so none of the batcher members is needed.
struct Toy : CodecBase {
    using Sample = float;
    struct Params {};
    struct Packet {
        std::uint64_t ts = 0;  // (CodecBase::id reads it)
        float value[4] = {0, 0, 0, 0};
    };
    explicit Toy(const Params &) {}
    static constexpr int kBatchKind = 0;
    std::size_t channels() const { return 1; }
    std::size_t packet_frames(std::size_t) const { return 4; }
    std::size_t plane_offset(std::size_t, std::size_t i, std::size_t) const { return i * 4; }
    void decode_batch(Context &, const std::vector<Packet> &batch, std::vector<float> &pcm) {
        ++calls;
        pcm.resize(batch.size() * 4);
        for (std::size_t i = 0; i < batch.size(); ++i) {
            for (std::size_t f = 0; f < 4; ++f) pcm[i * 4 + f] = batch[i].value[f] + carry_;
            carry_ = batch[i].value[3];
        }
    }
    static int calls;  // decode_batch calls of every Toy (the test has one)

private:
    float carry_ = 0.0f;
};
int Toy::calls = 0;

static_assert(Flac::kVerifies && Adpcm::kBlockInterleave && Pcm::kBlockInterleave && AacLc::kDirect, "the codecs that override a constant of the base");
static_assert(!Toy::kVerifies && !Toy::kBlockInterleave && !Toy::kDirect, "the base's constants");
static_assert(!AacLc::kVerifies && !Flac::kBlockInterleave && !Flac::kDirect, "a codec overrides only what it names");

int main() {
    Context ctx(0);
    std::vector<Toy::Packet> track(5);
    for (std::size_t i = 0; i < track.size(); ++i) {
        track[i].ts = 100 + 4 * i;
        for (std::size_t f = 0; f < 4; ++f) track[i].value[f] = (float)(10 * (i + 1) + f);
    }
    std::size_t cursor = 0;  // the demuxer's read position: decode(track[i]) is called with cursor == i + 1
    LookaheadDecoder<Toy> dec(ctx, Toy::Params{}, 2, [&]() -> std::optional<Toy::Packet> {
        if (cursor >= track.size()) return std::nullopt;
        return track[cursor++];
    });
    float carry = 0.0f;  // the frame-by-frame decoder
    auto step = [&](std::size_t i) {
        if (cursor <= i) cursor = i + 1;
        const AudioBufferRef &buf = dec.decode(track[i]);
        EXPECT(buf.frames == 4 && buf.planes.size() == 1, "buffer shape at packet %zu", i);
        for (std::size_t f = 0; f < 4 && buf.frames == 4; ++f)
            EXPECT(buf.planes[0][f] == track[i].value[f] + carry, "packet %zu frame %zu: %g, expected %g", i, f, (double)buf.planes[0][f], (double)(track[i].value[f] + carry));
        carry = track[i].value[3];
    };
    for (std::size_t i = 0; i < 3; ++i) step(i);  // batches {0, 1} and {2, 3}: packet 2 is across the boundary
    EXPECT(dec.batches_run() == 2 && Toy::calls == 2, "%zu batches in %d calls, expected 2 in 2", dec.batches_run(), Toy::calls);
    try {  // in mid-stream (packet 3 is computed and not handed out): refused for a codec that verifies, nothing at all for this one
        dec.set_verify(true);
    } catch (const std::exception &e) {
        EXPECT(false, "set_verify(true) in mid-stream threw: %s", e.what());
    }
    EXPECT(!dec.finalize().verify_ok.has_value(), "finalize() of a codec that verifies nothing has a verdict");
    EXPECT(dec.narrow_batches() == 0 && dec.wide_batches() == 0, "narrow / wide batches of a codec without an input format");
    // packet 3 is skipped without reset(): the carried state is already that of the end of the batch (after packet 3), and the replay of
    // packet 2 puts back what a frame-by-frame decoder, which never saw packet 3, carries
    cursor = 4;
    step(4);
    EXPECT(Toy::calls == 4 && dec.batches_run() == 3, "%d calls and %zu batches, expected 4 (one of them the replay) and 3", Toy::calls, dec.batches_run());
    dec.reset();
    EXPECT(dec.last_decoded().is_empty(), "reset() must clear the buffer");
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures ? 1 : 0;
}
