// What a launch of the batcher is built from (batcher.cpp is the only file that includes this): the shape of a kind's planes and of a
// submission's slot, the launch's view of a submission, the carver and the piece writer, and ONE HOME PER KIND THAT HAS LISTS --
// AacLists, VorbisLists, Mp3Lists: what the kind validates and counts over the views, the lists it requests from the carver, the lists
// of one chunk (re-based to the chunk's first chain / pair / step) with their copy pieces, and the chunk's kernels.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "symaccel_internal.h"

namespace symaccel {
namespace batch {

constexpr int kMaxIn = 6, kMaxState = 3;  // (symaccel_batch_slot's input[] / state[])
constexpr size_t kVorbisPosts = 65;      // floor1_Y values per channel-block in a VORBIS_DECODE submission (floor.rs:510-520)

inline size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t pieces_of(size_t bytes) { return (bytes + kBatchCopyPiece - 1) / kBatchCopyPiece; }

// what a kind's planes weigh: bytes per chain (per ticket for `in_per_ticket`, per `in_div` chains otherwise) for `units` frames /
// granules / blocks / words per chain
struct PlaneSizes {
    size_t in[kMaxIn] = {0, 0, 0, 0, 0, 0};
    bool in_per_ticket[kMaxIn] = {false, false, false, false, false, false};
    bool in_host_only[kMaxIn] = {false, false, false, false, false, false};  // read by the host when the group is launched; never copied as it is
    uint8_t in_div[kMaxIn] = {1, 1, 1, 1, 1, 1};                             // 2: one element per channel PAIR (chains 2p, 2p + 1)
    size_t state[kMaxState] = {0, 0, 0};
    uint8_t state_div = 1;  // k: the state planes hold one element per k chains (the verify forms of FLAC_RESTORE: one per frame)
    size_t out = 0;
    bool in_place = false;  // the result overwrites input[0] (FLAC / ALAC: the entry points they stand for work in place)
    int n_in = 0, n_state = 0;
    size_t out_per_chain() const { return in_place ? in[0] : out; }
};

// a submission's page-locked slot: [in 0 | .. | state 0 | .. | out], every plane on a 256-byte boundary (in place: out IS in 0)
struct SlotLayout {
    size_t in[kMaxIn] = {}, state[kMaxState] = {}, out = 0, bytes = 0;
    size_t in_bytes[kMaxIn] = {}, state_bytes[kMaxState] = {}, out_bytes = 0;
};

struct VorbisParam {  // `param`, decoded once per kind.  VORBIS_SYNTH / VORBIS_DECODE: e0 | e1 << 8 (| channels << 16)
    int e0, e1, nch;
    size_t cap;  // floats per chain of the spectrum and the PCM planes (a block has at most bs1 / 2 lines and yields at most bs1 / 2 samples)
};
inline VorbisParam vorbis_param(int param, size_t units) {
    const int e1 = (param >> 8) & 255;
    return {param & 255, e1, (param >> 16) & 255, e1 >= 1 && e1 <= 13 ? units << (e1 - 1) : 0};  // (lib.rs:404-406: a block has at most 8192 samples)
}
struct AdpcmParam {  // ADPCM_DECODE: codec | channels << 8 | out_fmt << 16 (the format joins inside the batcher: reserve_fmt)
    int codec, nch, fmt;
};
inline AdpcmParam adpcm_param(int param) { return {param & 255, (param >> 8) & 255, (param >> 16) & 255}; }
struct PcmDecParam {  // PCM_DECODE: codec | channels << 8 | shift << 16 | out_fmt << 24 (the format joins inside the batcher: reserve_fmt)
    int codec, nch, shift, fmt;
};
inline PcmDecParam pcmdec_param(int param) { return {param & 255, (param >> 8) & 255, (param >> 16) & 255, (param >> 24) & 15}; }
struct PairParam {  // FLAC_RESTORE: 0, or 0x100 | out_shift; ALAC_PREDICT: 0 or 0x100 -- the fused stereo forms
    bool pairs;
    uint32_t shift;
};
inline PairParam pair_param(int param) { return {(param & 0x300) == 0x100, (uint32_t)(param & 31)}; }
struct FlacVerifyParam {  // FLAC_RESTORE: 0x200 | (nch - 1) << 12, or 0x300 | out_shift | (nch - 1) << 12 -- restore, then the STREAMINFO MD5
    bool verify, finish;
    uint32_t shift;
    unsigned nch;
};
inline FlacVerifyParam flac_verify_param(int param) {
    return {(param & 0x200) != 0, (param & 0x300) == 0x300, (uint32_t)(param & 31), (param & 0x200) ? (unsigned)((param >> 12) & 7) + 1 : 1u};
}

// Vorbis: how much of a chain's spectrum / PCM plane its blocks fill (lines of the packed spectrum; samples of the packed PCM:
// lib.rs:303 -- a block yields (prev_n + n) / 4, the first block after a reset keeps n / 2 slots): only that much crosses the link
struct VorbisUsed {
    size_t lines, samples;
};
inline VorbisUsed vorbis_used(const uint8_t *flags, size_t nb, int32_t prev, int e0, int e1) {
    const size_t bs[2] = {(size_t)1 << e0, (size_t)1 << e1};
    VorbisUsed u{0, 0};
    int p = prev < 0 ? -1 : (prev ? 1 : 0);
    for (size_t i = 0; i < nb; ++i) {
        const int f = flags[i] ? 1 : 0;
        u.lines += bs[f] / 2;
        u.samples += p >= 0 ? (bs[p] + bs[f]) / 4 : bs[f] / 2;
        p = f;
    }
    return u;
}

// what a launch needs of a submission: copied out of the ticket table when the group closes, because the launch runs outside the
// batcher's mutex and the table may grow meanwhile; `lay` and `used` are filled in front of the first chunk (so nothing depends on
// what a chunk's scatter leaves in the slot's state planes)
struct TicketView {
    char *slot = nullptr;
    uint32_t first_chain = 0, n_chains = 0;
    int status = SYMACCEL_OK;
    int out_fmt = 0;
    uint32_t channels = 0;
    size_t out_valid = 0;
    int in_fmt = 0;                // 0, or SYMACCEL_FMT_S16: plane 0 of the slot holds int16_t words (FLAC_RESTORE / ALAC_PREDICT, symaccel_batcher_reserve_io);
                                   // or SYMACCEL_IN_FMT_ROWS: every row at its native offset, at row_bytes()[row] bytes a word
    int fmt_status = SYMACCEL_OK;  // what the output format has to say about the submission (Vorbis: an interleave group whose chains disagree)
    SlotLayout lay;
    const VorbisUsed *used = nullptr;  // the two Vorbis kinds: what the blocks of chain c fill, used[c]
    template <class T> T *in(int i) const { return reinterpret_cast<T *>(slot + lay.in[i]); }
    template <class T> T *state(int i) const { return reinterpret_cast<T *>(slot + lay.state[i]); }
    // SYMACCEL_IN_FMT_ROWS: the width table (slot.input[5]), behind the planes every ticket of the shape has; read by the host only
    const uint8_t *row_bytes() const { return reinterpret_cast<const uint8_t *>(slot + lay.bytes); }
};

// chains [c0, c0 + nc) = submissions [t0, t0 + nt) of a group, and where their planes start on the device
struct Chunk {
    size_t c0, nc, t0, nt;
    char *in[kMaxIn], *si[kMaxState], *so[kMaxState], *out;
};

// A bump carver (the idiom of stage.cpp's Pipe::alloc / commit): every plane or list is requested once with its size, in ONE walk
// that is taken twice -- without memory (base = nullptr) for `total`, what the memory must hold, then over the memory for the pointers.
struct Carver {
    char *base = nullptr;
    size_t total = 0;
    template <class T> void want(T **p, size_t bytes) {
        *p = base ? reinterpret_cast<T *>(base + total) : nullptr;
        total += round256(bytes);
    }
};
// a list the host builds (page-locked, behind the copy descriptors) and the device mirrors
template <class T> void want_both(Carver &dev, Carver &host, T **d, T **h, size_t bytes) {
    dev.want(d, bytes);
    host.want(h, bytes);
}

// The copy pieces of a launch, written into the descriptor area [w, end): the area holds what piece_bound() (batcher.cpp) says a launch
// can need at most; a piece beyond it is NOT written and sets `overflow`, which fails the launch.
// A bulk plane (a submission's spectra, its PCM) of `dma_bytes` or more goes through a copy ENGINE (hipMemcpyAsync on the lane's copy
// stream) instead of the piece list: the engines move large PCIe payloads, a kernel's 64-byte accesses pay a header per 64 bytes
// in both directions -- two kernels copying against each other reached 30 + 30 GB/s, the engines 44 + 44 (profiles/r06d_*).  The
// small planes of a chunk (records, state, lists) still share ONE gather / scatter launch.
struct Pieces {
    BatchCopyDesc *w, *end;
    size_t dma_bytes;
    bool overflow = false;
    struct Dma {
        const char *src;
        char *dst;
        size_t bytes;
    };
    std::vector<Dma> dma;
    void piece(const void *src, void *dst, size_t bytes, uint32_t pad) {
        if (w == end) overflow = true;
        else *w++ = BatchCopyDesc{src, dst, (uint32_t)bytes, pad};
    }
    void add(const void *src, void *dst, size_t bytes) {
        for (size_t o = 0; o < bytes; o += kBatchCopyPiece)
            piece(static_cast<const char *>(src) + o, static_cast<char *>(dst) + o, std::min(kBatchCopyPiece, bytes - o), 0);
    }
    // int16_t words of a slot -> int32_t words of the device plane: cut by the DESTINATION's bytes, so that a narrow plane is as many
    // pieces as the same plane sent wide (piece_bound() counts it as that); never through a copy engine, which cannot widen
    // (word_bytes 3: packed 24-bit words, a row of a ticket with a width per row; a piece of 4096 words then starts 12 288 bytes behind
    // the last, so every piece of a row keeps the row's alignment modulo 16)
    void widen(const char *src, char *dst, size_t dst_bytes, unsigned word_bytes = 2) {
        for (size_t o = 0; o < dst_bytes; o += kBatchCopyPiece)
            piece(src + o / 4 * word_bytes, dst + o, std::min(kBatchCopyPiece, dst_bytes - o), batch_piece_widen(word_bytes));
    }
    void bulk(const char *src, char *dst, size_t bytes) {
        if (dma_bytes && bytes >= dma_bytes) dma.push_back({src, dst, bytes});
        else add(src, dst, bytes);
    }
};

// ------------------------------------------------------------------------------------------------ MP3_DECODE
// unit_chains of every submission (its one or two chains), relative to the first chain of the chunk the submission falls into
struct Mp3Lists {
    int32_t *d_units = nullptr, *h_units = nullptr;
    void request(Carver &dev, Carver &host, size_t tickets) { want_both(dev, host, &d_units, &h_units, tickets * 8); }
    void build(const std::vector<TicketView> &views, const Chunk &ch, Pieces &pw) {
        for (size_t ti = ch.t0; ti < ch.t0 + ch.nt; ++ti) {
            const int32_t rel = (int32_t)(views[ti].first_chain - ch.c0);
            h_units[2 * ti] = rel;
            h_units[2 * ti + 1] = views[ti].n_chains == 2 ? rel + 1 : -1;
        }
        pw.add(h_units + 2 * ch.t0, d_units + 2 * ch.t0, ch.nt * 8);
    }
    int run(symaccel_ctx *ctx, const Chunk &ch, int param, size_t units) const {
        return launch_mp3_decode(ctx, (const int16_t *)ch.in[0], (const symaccel_mp3_requant *)ch.in[1], d_units + 2 * ch.t0,
                                 (const symaccel_mp3_stereo *)ch.in[3], ch.nt, (const symaccel_mp3_side *)ch.in[2], param, (const float *)ch.si[0],
                                 (const float *)ch.si[1], (const int32_t *)ch.si[2], (float *)ch.so[0], (float *)ch.so[1], (int32_t *)ch.so[2],
                                 (float *)ch.out, ch.nc, units);
    }
};

// ------------------------------------------------------------------------------------------------ FLAC_RESTORE, the verify forms
// One symaccel_flac_md5_job per submission (a submission is one stream's run of frames): its rows in the device plane at the group's
// pitch, its ranges of the frame plane (in[3]) and of the two state planes -- the starting state is entry 0 of the plane that went in,
// the checkpoints fill the plane that goes back.  A submission that failed gets state = NULL: the kernel skips it.
struct FlacVerifyLists {
    symaccel_flac_md5_job *d_jobs = nullptr, *h_jobs = nullptr;
    void request(Carver &dev, Carver &host, size_t tickets) { want_both(dev, host, &d_jobs, &h_jobs, tickets * sizeof(symaccel_flac_md5_job)); }
    void build(const std::vector<TicketView> &views, const Chunk &ch, unsigned nch, char *d_rows, size_t pitch_bytes, char *d_frames, char *d_state_in,
               char *d_state_out, Pieces &pw) {
        for (size_t ti = ch.t0; ti < ch.t0 + ch.nt; ++ti) {
            const TicketView &t = views[ti];
            const size_t f0 = t.first_chain / nch;
            symaccel_flac_md5_job j{};
            j.rows = reinterpret_cast<const int32_t *>(d_rows + (size_t)t.first_chain * pitch_bytes);
            j.frames = reinterpret_cast<const symaccel_flac_md5_frame *>(d_frames) + f0;
            j.state = t.status == SYMACCEL_OK ? reinterpret_cast<symaccel_md5_state *>(d_state_in) + f0 : nullptr;
            j.checkpoints = reinterpret_cast<symaccel_md5_state *>(d_state_out) + f0;
            j.row_pitch = pitch_bytes / 4;
            j.n_frames = t.n_chains / nch;
            j.nch = (uint8_t)nch;
            j.bytes_per_sample = 0;  // (every frame names its own: check_flac)
            h_jobs[ti] = j;
        }
        pw.add(h_jobs + ch.t0, d_jobs + ch.t0, ch.nt * sizeof(symaccel_flac_md5_job));
    }
    int run(symaccel_ctx *ctx, const Chunk &ch, bool finish, uint32_t shift) const { return launch_flac_md5(ctx, d_jobs + ch.t0, ch.nt, finish, shift); }
};

// ------------------------------------------------------------------------------------------------ AAC_DECODE
// The descriptor blob of an AAC_DECODE submission (plane in[2], n_chains * ps.in[2] bytes): what symaccel_aac_decode_pipelined takes
// beside the spectra -- [AacBlobHeader][pair_chains: n_pairs x 2 i32, chains of THIS submission][js rows: n_pairs x units x 644 B]
// [TNS filters: n_tns x 92 B, frame = chain * units + frame inside this submission]
struct AacBlobHeader {
    uint32_t n_pairs, n_tns, pad[2];
};
inline size_t aac_blob_pairs(size_t) { return sizeof(AacBlobHeader); }
inline size_t aac_blob_js(size_t n_pairs) { return sizeof(AacBlobHeader) + ((n_pairs * 8 + 15) & ~(size_t)15); }
inline size_t aac_blob_tns(size_t n_pairs, size_t units) { return aac_blob_js(n_pairs) + ((n_pairs * units * sizeof(symaccel_aac_js_frame) + 15) & ~(size_t)15); }
inline size_t aac_blob_bytes(size_t n_pairs, size_t units, size_t n_tns) { return aac_blob_tns(n_pairs, units) + n_tns * sizeof(symaccel_aac_tns_filter); }

// the group's pair list, joint-stereo rows, TNS filters, the pair frames that carry TNS, the walk's chain index
struct AacLists {
    AacBandMaps maps{};              // the band tables `param` names (copied when the group closes)
    size_t n_pairs = 0, n_tns = 0;  // totals of the group (count())
    int32_t *d_pairs = nullptr, *h_pairs = nullptr;
    symaccel_aac_tns_filter *d_tns = nullptr, *h_tns = nullptr;
    uint32_t *d_pf = nullptr, *h_pf = nullptr;
    symaccel_aac_js_frame *d_js = nullptr;
    void *d_index = nullptr;
    size_t p = 0, f = 0, q = 0;  // pairs / filters / TNS pair frames placed so far
    struct {                      // the chunk being launched: first pair / filter / TNS pair frame and their counts
        size_t p0, np, f0, nf, q0, nq;
    } chunk{};
    std::vector<uint8_t> seen;  // (scratch)
    std::vector<int32_t> pair_of;

    // what a submission's blob says, judged alone (its neighbours in the launch are not failed for it)
    int check(const PlaneSizes &ps, size_t units, const TicketView &v) {
        const AacBlobHeader *h = v.in<const AacBlobHeader>(2);
        if (2 * (size_t)h->n_pairs > v.n_chains || aac_blob_bytes(h->n_pairs, units, h->n_tns) > ps.in[2] * v.n_chains) return SYMACCEL_ERR_INVALID_ARG;
        const int32_t *pc = reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(h) + aac_blob_pairs(h->n_pairs));
        seen.assign(v.n_chains, 0);
        for (uint32_t i = 0; i < 2 * h->n_pairs; ++i) {
            const int32_t c = pc[i];
            if (c < 0 || (size_t)c >= v.n_chains || seen[(size_t)c]) return SYMACCEL_ERR_INVALID_ARG;
            seen[(size_t)c] = 1;
        }
        return SYMACCEL_OK;
    }
    // a blob that does not add up is neutralised (it runs as an empty description, its ticket fails) and the rest of the launch goes ahead
    void count(std::vector<TicketView> &views, const PlaneSizes &ps, size_t units, int param) {
        n_pairs = n_tns = p = f = q = 0;
        for (TicketView &v : views) {
            AacBlobHeader *h = v.in<AacBlobHeader>(2);
            v.status = check(ps, units, v);
            if (v.status == SYMACCEL_OK && h->n_pairs && param < 0) v.status = SYMACCEL_ERR_INVALID_ARG;  // (pairs need a band table)
            if (v.status != SYMACCEL_OK) h->n_pairs = h->n_tns = 0;
            n_pairs += h->n_pairs;
            n_tns += h->n_tns;
        }
    }
    void request(Carver &dev, Carver &host, size_t chains, size_t units) {
        want_both(dev, host, &d_pairs, &h_pairs, std::max<size_t>(1, n_pairs) * 8);
        dev.want(&d_js, std::max<size_t>(1, n_pairs) * units * sizeof(symaccel_aac_js_frame));
        want_both(dev, host, &d_tns, &h_tns, std::max<size_t>(1, n_tns) * sizeof(symaccel_aac_tns_filter));
        want_both(dev, host, &d_pf, &h_pf, std::max<size_t>(1, n_tns) * 4);
        dev.want(&d_index, aac_js_scratch_bytes(chains, n_pairs, units));
    }
    // the blobs of the chunk's submissions are taken apart: joint-stereo rows go as they are, the pair list and the filters are re-based
    // to the chunk (chain index relative to the chunk's first chain, pair index relative to its first pair)
    void build(const std::vector<TicketView> &views, const Chunk &ch, size_t units, Pieces &pw) {
        chunk = {p, 0, f, 0, q, 0};
        for (size_t ti = ch.t0; ti < ch.t0 + ch.nt; ++ti) {
            const TicketView &t = views[ti];
            const char *blob = t.in<const char>(2);
            const AacBlobHeader *h = reinterpret_cast<const AacBlobHeader *>(blob);
            const int32_t rel = (int32_t)(t.first_chain - ch.c0);
            const int32_t *pc = reinterpret_cast<const int32_t *>(blob + aac_blob_pairs(h->n_pairs));
            pair_of.assign(t.n_chains, -1);
            for (uint32_t i = 0; i < h->n_pairs; ++i) {
                const int32_t a = pc[2 * i], bb = pc[2 * i + 1];  // (in range and distinct: check())
                pair_of[(size_t)a] = pair_of[(size_t)bb] = (int32_t)i;
                h_pairs[2 * (p + i)] = rel + a;
                h_pairs[2 * (p + i) + 1] = rel + bb;
            }
            pw.add(blob + aac_blob_js(h->n_pairs), d_js + p * units, (size_t)h->n_pairs * units * sizeof(symaccel_aac_js_frame));
            const symaccel_aac_tns_filter *tf = reinterpret_cast<const symaccel_aac_tns_filter *>(blob + aac_blob_tns(h->n_pairs, units));
            for (uint32_t i = 0; i < h->n_tns; ++i) {
                symaccel_aac_tns_filter flt = tf[i];
                const size_t chain = flt.frame / units, frame = flt.frame % units;
                if (chain >= t.n_chains) flt.frame = 0xffffffffu;  // (what symaccel_aac_tns_device skips)
                else flt.frame = (uint32_t)(((size_t)rel + chain) * units + frame);
                h_tns[f++] = flt;
                if (chain < t.n_chains && pair_of[chain] >= 0)  // a pair frame with TNS: joint stereo first, in place (list pass)
                    h_pf[q++] = (uint32_t)((p - chunk.p0 + (size_t)pair_of[chain]) * units + frame);
            }
            p += h->n_pairs;
        }
        // (a pair frame listed twice -- both channels carry filters -- would be decoded twice: the list is made unique)
        std::sort(h_pf + chunk.q0, h_pf + q);
        q = (size_t)(std::unique(h_pf + chunk.q0, h_pf + q) - h_pf);
        chunk.np = p - chunk.p0;
        chunk.nf = f - chunk.f0;
        chunk.nq = q - chunk.q0;
        pw.add(h_pairs + 2 * chunk.p0, d_pairs + 2 * chunk.p0, chunk.np * 8);
        pw.add(h_tns + chunk.f0, d_tns + chunk.f0, chunk.nf * sizeof(symaccel_aac_tns_filter));
        pw.add(h_pf + chunk.q0, d_pf + chunk.q0, chunk.nq * 4);
    }
    // symaccel_aac_decode_pipelined's kernel sequence (csrc/stage.cpp) on the chunk: the pair frames that carry TNS get their joint
    // stereo decoded in place (a list pass), the filters run, ONE walk decodes the joint stereo of every other frame on load
    int run(symaccel_ctx *ctx, const Chunk &ch, size_t units) const {
        const int32_t *pairs = d_pairs + 2 * chunk.p0;
        symaccel_aac_js_frame *js = d_js + chunk.p0 * units;
        if (chunk.nq) {
            SYM_TRY(launch_aac_joint_stereo(ctx, maps, (float *)ch.in[0], units, pairs, js, chunk.np, d_pf + chunk.q0, chunk.nq));
            SYM_TRY(launch_aac_js_consume(ctx, js, d_pf + chunk.q0, chunk.nq, chunk.np * units));
        }
        if (chunk.nf) SYM_TRY(launch_aac_tns(ctx, (float *)ch.in[0], ch.nc * units, d_tns + chunk.f0, chunk.nf));
        return launch_aac(ctx, (const float *)ch.in[0], (const uint8_t *)ch.in[1], (const float *)ch.si[0], (float *)ch.so[0], (float *)ch.out, ch.nc, units,
                          chunk.np ? &maps : nullptr, pairs, js, chunk.np, d_index);
    }
};

// ------------------------------------------------------------------------------------------------ VORBIS_DECODE
// coupling steps a block may carry in a VORBIS_DECODE submission: every ordered channel pair once, at least 8 (a mapping may list up to
// 256 steps, lib.rs:604-640 -- a stream with more than this per block keeps batching per stream through symaccel_vorbis_decode)
inline size_t vorbis_max_steps(size_t nch) { return std::min<size_t>(256, std::max<size_t>(8, nch * (nch - 1))); }
// The coupling blob of a VORBIS_DECODE submission (plane in[4]): first[units + 1] u32 -- the steps of block b are
// [first[b], first[b + 1]) --, padded to 16 bytes, then the steps as (magnitude channel, angle channel) byte pairs
inline size_t vorbis_blob_steps(size_t units) { return ((units + 1) * 4 + 15) & ~(size_t)15; }

// the byte plane of the floor curves, the floor1_Y rows and line offsets by (configuration, block size) class, the blocks' line
// offsets, the channel-blocks without a floor, the coupling steps
struct VorbisLists {
    std::vector<symaccel_vorbis_floor1_cfg> floors;  // the registered configurations (copied when the group closes)
    size_t n_steps = 0;                              // coupling steps of the group (count())
    struct {                                         // bytes of the group's lists (count())
        size_t ys, offs, boff, kill, first, steps;
    } bytes{};
    uint8_t *d_plane = nullptr, *d_kill = nullptr, *h_kill = nullptr, *d_steps = nullptr, *h_steps = nullptr;
    uint32_t *d_ys = nullptr, *h_ys = nullptr, *d_offs = nullptr, *h_offs = nullptr, *d_boff = nullptr, *h_boff = nullptr, *d_first = nullptr, *h_first = nullptr;
    size_t first_at = 0, steps_at = 0, ys_at = 0, offs_at = 0;  // placed so far
    struct Class {
        uint32_t cfg, n2;
        size_t ys0, offs0, count;
    };
    struct {  // the chunk being launched
        std::vector<Class> classes;
        size_t boff0, kill0, first0, steps0, n_steps;
        bool prepare;
    } chunk{};
    std::vector<uint32_t> count_of;  // (scratch: channel-blocks per class, where the next row of a class goes)
    std::vector<size_t> ys_next, offs_next;
    std::vector<symaccel_vorbis_floor1_job> jobs;

    // a submission, judged alone (what symaccel_vorbis_decode checks of a stream); *steps = its coupling steps
    int check(const PlaneSizes &ps, size_t nb, const TicketView &v, size_t *steps) const {
        const size_t nch = v.n_chains;
        const uint8_t *flags = v.in<const uint8_t>(1), *floor = v.in<const uint8_t>(2);
        const uint32_t *posts = v.in<const uint32_t>(3);
        const int32_t *prev = v.state<const int32_t>(0);
        *steps = 0;
        // the channels of a stream share their block flags and their previous flag (one mode per packet, lib.rs:170-178)
        for (size_t c = 1; c < nch; ++c) {
            if (prev[c] != prev[0]) return SYMACCEL_ERR_INVALID_ARG;
            for (size_t b = 0; b < nb; ++b)
                if ((flags[c * nb + b] != 0) != (flags[b] != 0)) return SYMACCEL_ERR_INVALID_ARG;
        }
        for (size_t cb = 0; cb < nch * nb; ++cb) {
            const unsigned fl = floor[cb];
            if (fl == SYMACCEL_VORBIS_FLOOR_UNUSED) continue;
            if (fl >= floors.size()) return SYMACCEL_ERR_INVALID_ARG;
            const uint32_t *y = posts + cb * kVorbisPosts;
            for (unsigned i = 0; i < floors[fl].n_posts; ++i)
                if (y[i] > 511u) return SYMACCEL_ERR_UNSUPPORTED;  // (symaccel_vorbis_floor1_status_device's domain)
        }
        const uint32_t *first = v.in<const uint32_t>(4);
        const uint8_t *st = v.in<const uint8_t>(4) + vorbis_blob_steps(nb);
        if (first[0] != 0) return SYMACCEL_ERR_INVALID_ARG;
        for (size_t b = 0; b < nb; ++b)
            if (first[b + 1] < first[b]) return SYMACCEL_ERR_INVALID_ARG;
        const size_t n = first[nb];
        if (vorbis_blob_steps(nb) + 2 * n > ps.in[4]) return SYMACCEL_ERR_INVALID_ARG;
        for (size_t s = 0; s < n; ++s)
            if (st[2 * s] >= nch || st[2 * s + 1] >= nch || st[2 * s] == st[2 * s + 1]) return SYMACCEL_ERR_INVALID_ARG;  // lib.rs:253
        *steps = n;
        return SYMACCEL_OK;
    }
    void count(std::vector<TicketView> &views, const PlaneSizes &ps, size_t nb, size_t chains) {
        n_steps = first_at = steps_at = ys_at = offs_at = 0;
        for (TicketView &v : views) {
            size_t steps = 0;
            v.status = check(ps, nb, v, &steps);
            n_steps += steps;
        }
        bytes.ys = round256(chains * nb * kVorbisPosts * 4);
        bytes.offs = round256(chains * nb * 4);
        bytes.boff = round256(views.size() * (nb + 1) * 4);
        bytes.kill = round256(chains * nb);
        bytes.first = round256((views.size() * (nb + 1) + 1) * 4);  // (every chunk's list starts with a 0 of its own)
        bytes.steps = round256(std::max<size_t>(1, n_steps) * 2);
    }
    void request(Carver &dev, Carver &host, size_t chains, size_t cap) {
        dev.want(&d_plane, chains * cap);  // one byte per line
        want_both(dev, host, &d_ys, &h_ys, bytes.ys);
        want_both(dev, host, &d_offs, &h_offs, bytes.offs);
        want_both(dev, host, &d_boff, &h_boff, bytes.boff);
        want_both(dev, host, &d_kill, &h_kill, bytes.kill);
        want_both(dev, host, &d_first, &h_first, bytes.first);
        want_both(dev, host, &d_steps, &h_steps, bytes.steps);
    }
    // The chunk's streams in symaccel_vorbis_decode's terms: where every block's lines start, which channel-blocks have no floor,
    // the coupling steps block by block (this half); per (floor configuration, block size) class the floor1_Y rows and the byte
    // offsets of their lines in the chunk's plane (build_classes)
    void build(const std::vector<TicketView> &views, const Chunk &ch, const VorbisParam &vp, size_t nb, Pieces &pw) {
        const size_t nch = (size_t)vp.nch;
        chunk.classes.clear();
        chunk.boff0 = ch.t0 * (nb + 1);
        chunk.kill0 = ch.c0 * nb;
        chunk.first0 = first_at;
        chunk.steps0 = steps_at;
        bool any_kill = false;
        count_of.assign(512, 0);
        h_first[first_at] = 0;
        for (size_t ti = ch.t0; ti < ch.t0 + ch.nt; ++ti) {
            const TicketView &t = views[ti];
            const uint8_t *flags = t.in<const uint8_t>(1), *floor = t.in<const uint8_t>(2);
            uint32_t *boff = h_boff + ti * (nb + 1);
            size_t lines = 0;
            for (size_t b = 0; b < nb; ++b) {
                boff[b] = (uint32_t)lines;
                lines += (size_t)1 << ((flags[b] ? vp.e1 : vp.e0) - 1);
            }
            boff[nb] = (uint32_t)lines;
            const bool ok = t.status == SYMACCEL_OK;
            for (size_t c = 0; c < nch; ++c)
                for (size_t b = 0; b < nb; ++b) {
                    const unsigned fl = ok ? floor[c * nb + b] : SYMACCEL_VORBIS_FLOOR_UNUSED;
                    const bool kill = fl == SYMACCEL_VORBIS_FLOOR_UNUSED;
                    h_kill[((size_t)t.first_chain + c) * nb + b] = kill ? 1 : 0;
                    any_kill |= kill;
                    if (!kill) count_of[2 * fl + (flags[b] ? 1 : 0)] += 1;
                }
            // the steps: block by block behind the chunk's list (a failed submission has none)
            const uint32_t *first = t.in<const uint32_t>(4);
            const uint8_t *st = t.in<const uint8_t>(4) + vorbis_blob_steps(nb);
            uint32_t *out_first = h_first + first_at + (ti - ch.t0) * nb;
            const uint32_t base = out_first[0];
            for (size_t b = 0; b < nb; ++b) out_first[b + 1] = base + (ok ? first[b + 1] : 0);
            if (ok && first[nb]) std::memcpy(h_steps + 2 * (steps_at + base), st, 2 * (size_t)first[nb]);
        }
        chunk.n_steps = h_first[first_at + ch.nt * nb];
        chunk.prepare = chunk.n_steps != 0 || any_kill;
        if (chunk.prepare) {
            pw.add(h_boff + chunk.boff0, d_boff + chunk.boff0, ch.nt * (nb + 1) * 4);
            pw.add(h_kill + chunk.kill0, d_kill + chunk.kill0, ch.nc * nb);
            pw.add(h_first + chunk.first0, d_first + chunk.first0, (ch.nt * nb + 1) * 4);
            pw.add(h_steps + 2 * chunk.steps0, d_steps + 2 * chunk.steps0, 2 * chunk.n_steps);
        }
        first_at += ch.nt * nb + 1;
        steps_at += chunk.n_steps;
        build_classes(views, ch, vp, nb, pw);
    }
    // classes in (configuration, block size) order, their rows behind each other (count_of: build())
    void build_classes(const std::vector<TicketView> &views, const Chunk &ch, const VorbisParam &vp, size_t nb, Pieces &pw) {
        const size_t nch = (size_t)vp.nch, ys_begin = ys_at, offs_begin = offs_at;
        ys_next.assign(512, 0);
        offs_next.assign(512, 0);
        for (size_t kc = 0; kc < 512; ++kc) {
            if (!count_of[kc]) continue;
            ys_next[kc] = ys_at;
            offs_next[kc] = offs_at;
            chunk.classes.push_back({(uint32_t)(kc / 2), (uint32_t)1 << ((kc & 1 ? vp.e1 : vp.e0) - 1), ys_at, offs_at, count_of[kc]});
            ys_at += (size_t)count_of[kc] * floors[kc / 2].n_posts;
            offs_at += count_of[kc];
        }
        for (size_t ti = ch.t0; ti < ch.t0 + ch.nt; ++ti) {
            const TicketView &t = views[ti];
            if (t.status != SYMACCEL_OK) continue;
            const uint8_t *flags = t.in<const uint8_t>(1), *floor = t.in<const uint8_t>(2);
            const uint32_t *posts = t.in<const uint32_t>(3), *boff = h_boff + ti * (nb + 1);
            for (size_t c = 0; c < nch; ++c)
                for (size_t b = 0; b < nb; ++b) {
                    const unsigned fl = floor[c * nb + b];
                    if (fl == SYMACCEL_VORBIS_FLOOR_UNUSED) continue;
                    const size_t kc = 2 * fl + (flags[b] ? 1 : 0);
                    const unsigned np = floors[fl].n_posts;
                    std::memcpy(h_ys + ys_next[kc], posts + (c * nb + b) * kVorbisPosts, np * 4);
                    ys_next[kc] += np;
                    h_offs[offs_next[kc]++] = (uint32_t)(((size_t)t.first_chain - ch.c0 + c) * vp.cap + boff[b]);
                }
        }
        pw.add(h_ys + ys_begin, d_ys + ys_begin, (ys_at - ys_begin) * 4);
        pw.add(h_offs + offs_begin, d_offs + offs_begin, (offs_at - offs_begin) * 4);
    }
    // symaccel_vorbis_decode's kernel sequence (csrc/ctx.cpp) on the chunk: the coupling steps and the zero floors in place
    // (lib.rs:250-278, 206-209), the floor curves as one byte per line -- the (configuration, block size) classes two per launch
    // (floor.rs:568-653, 776-825) --, then the synthesis with table[y] * residue in its load path (lib.rs:282-292, dsp.rs:68-126)
    int run(symaccel_ctx *ctx, const Chunk &ch, const VorbisParam &vp, size_t nb) {
        uint8_t *plane = d_plane + ch.c0 * vp.cap;
        SYM_GPU(ctx, hipMemsetAsync(plane, 0, ch.nc * vp.cap, ctx->stream));
        if (chunk.prepare)
            SYM_TRY(launch_vorbis_prepare(ctx, (float *)ch.in[0], vp.cap, (unsigned)vp.nch, ch.nt, nb, d_boff + chunk.boff0, d_steps + 2 * chunk.steps0,
                                          d_first + chunk.first0, d_kill + chunk.kill0));
        jobs.clear();  // two classes per launch
        for (const Class &k : chunk.classes) {
            const symaccel_vorbis_floor1_cfg &cfg = floors[k.cfg];
            jobs.push_back(symaccel_vorbis_floor1_job{cfg.x_list, cfg.n_posts, cfg.multiplier, d_ys + k.ys0, k.n2, d_offs + k.offs0, k.count});
        }
        SYM_TRY(symaccel_vorbis_floor1_y_jobs_device(ctx, jobs.data(), jobs.size(), plane));
        return symaccel_vorbis_synth_fy_pp_device(ctx, vp.e0, vp.e1, plane, (const float *)ch.in[0], vp.cap, (const uint8_t *)ch.in[1], (const int32_t *)ch.si[0],
                                                  (int32_t *)ch.so[0], (const float *)ch.si[1], (float *)ch.so[1], (float *)ch.out, vp.cap, ch.nc, nb);
    }
};

}  // namespace batch
}  // namespace symaccel
