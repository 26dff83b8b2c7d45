// Cross-stream batcher: many decoders, one launch.
//
// A `Hip*Decoder` (bindings/rust) or a `codecs::LookaheadDecoder` (include/symaccel.hpp) batches the look-ahead of ITS stream:
// 256 packets x 2 channels is 2 MiB per call, and N decoders are N small calls, each paying its own launch and its own PCIe
// round trip.  The reference's trait gives a decoder no view of its siblings (AudioDecoder::decode_ref sees one packet of one
// track, symphonia-core/src/codecs/audio.rs:279-297; the registry builds decoders from (params, opts) alone, registry.rs:330-341),
// so the coalescing point is below the trait, here: decoders SUBMIT their batches to a batcher shared by the process and come
// back for the result later; whatever is pending when somebody needs a result (or when `flush_bytes` of input have piled up)
// goes to the device as ONE batch per (kind, param, units per chain) group -- the chains of every submission side by side in the
// chain-major layout the kernels already take, so nothing in the kernels knows about streams.
//
//   reserve()  -> a slot of page-locked staging memory the front end writes its spectra / samples / records into (no copy
//                 between the parser's output and the DMA source) + a ticket
//   commit()   -> the slot is filled
//   wait()     -> launches the ticket's group if nobody has yet (and everything else that is pending), blocks until the
//                 group's results are in page-locked memory; slot.out / slot.state now hold PCM and the carried state
//   release()  -> the slot may be reused
//
// A group is transferred and transformed in chunks of submissions: gather(c + 1) || kernel(c) || scatter(c - 1) on the three
// streams of a LANE (the chunks are chains, which are independent: no carried state between chunks, unlike stage.cpp's
// frame-axis chunks).  A lane is a context of its own (stream, scratch, tables) plus two copy streams and a mutex; a group that
// closes is handed to the next lane and ENQUEUED OUTSIDE the batcher's mutex -- the threads of other streams keep reserving,
// committing and collecting while one thread builds the copy descriptors and launches, and the gather of one group overlaps the
// scatter of another on a different lane.  Groups are pooled: in the steady state nothing is allocated.  Thread-safe: submissions
// may come from any thread; a flush waits for reservations of the group that are still being filled.  The status of a launch is
// kept PER TICKET: a submission whose descriptors do not add up fails alone, its neighbours in the launch succeed.  A context that
// has a batcher is driven through the batcher only (the context itself is externally synchronised, include/symaccel.h "Thread safety").
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "batcher_lists.h"

using namespace symaccel;
using namespace symaccel::batch;

namespace {

bool plane_sizes(int kind, int param, size_t units, PlaneSizes *ps) {
    *ps = PlaneSizes();
    switch (kind) {
    case SYMACCEL_BATCH_AAC_SYNTH:   // symaccel_aac_synth: coeffs, side | delay | pcm
    case SYMACCEL_BATCH_AAC_DECODE:  // symaccel_aac_decode_pipelined for one stream: coeffs, side, the stream's descriptor blob | delay | pcm
        ps->n_in = 2;
        ps->in[0] = units * 4096;
        ps->in[1] = units;
        if (kind == SYMACCEL_BATCH_AAC_DECODE) {
            // the blob (aac_blob_*): header + pair list + joint-stereo rows (at most one pair per two chains) + TNS filters (at most
            // eight per channel-frame: one per window of an EIGHT_SHORT frame), sized per chain so that it scales with the stream
            ps->n_in = 3;
            ps->in[2] = 64 + units * (sizeof(symaccel_aac_js_frame) / 2 + 8 * sizeof(symaccel_aac_tns_filter));
            ps->in_host_only[2] = true;
        }
        ps->n_state = 1;
        ps->state[0] = 4096;
        ps->out = units * 4096;
        return true;
    case SYMACCEL_BATCH_VORBIS_SYNTH:     // symaccel_vorbis_synth with every chain's planes at their largest: spectra, flags | prev, overlap | pcm
    case SYMACCEL_BATCH_VORBIS_DECODE: {  // symaccel_vorbis_decode for ONE stream: residue, flags, floor index, posts, coupling blob | prev, overlap | pcm
        const bool decode = kind == SYMACCEL_BATCH_VORBIS_DECODE;
        const VorbisParam vp = vorbis_param(param, units);
        if (vp.e0 < 6 || vp.e1 > 13 || vp.e0 > vp.e1) return false;  // (the block sizes a Vorbis stream can have, lib.rs:404-406)
        if (decode ? vp.nch < 1 || (param >> 24) : (param >> 16)) return false;
        const size_t half = (size_t)1 << (vp.e1 - 1);
        ps->n_in = 2;
        ps->in[0] = units * half * 4;  // a block has at most bs1 / 2 lines ...
        ps->in[1] = units;
        if (decode) {
            ps->n_in = 5;
            ps->in[2] = units;  // floor configuration of every channel-block (symaccel_batcher_vorbis_floor's index), or ..._FLOOR_UNUSED
            ps->in[3] = units * kVorbisPosts * 4;
            // the coupling steps of the stream's blocks: first[units + 1] u32, padded to 16 bytes, then (magnitude, angle) byte pairs
            ps->in[4] = vorbis_blob_steps(units) + units * 2 * vorbis_max_steps((size_t)vp.nch);
            ps->in_per_ticket[4] = true;
            ps->in_host_only[2] = ps->in_host_only[3] = ps->in_host_only[4] = true;
        }
        ps->n_state = 2;
        ps->state[0] = 4;
        ps->state[1] = half * 4;
        ps->out = units * half * 4;  // ... and yields at most bs1 / 2 samples
        return true;
    }
    case SYMACCEL_BATCH_MP3_SYNTH:   // symaccel_mp3_synth: xr, side | overlap, vvec, vfront | pcm
    case SYMACCEL_BATCH_MP3_DECODE:  // symaccel_mp3_decode_pipelined, one stream per submission: quant, rq_desc, side, st_desc (per stream) | the same
        if (kind == SYMACCEL_BATCH_MP3_SYNTH) {
            ps->n_in = 2;
            ps->in[0] = units * 2304;
            ps->in[1] = units * sizeof(symaccel_mp3_side);
        } else {
            ps->n_in = 4;
            ps->in[0] = units * 1152;
            ps->in[1] = units * sizeof(symaccel_mp3_requant);
            ps->in[2] = units * sizeof(symaccel_mp3_side);
            ps->in[3] = units * sizeof(symaccel_mp3_stereo);
            ps->in_per_ticket[3] = true;
        }
        ps->n_state = 3;
        ps->state[0] = 2304;
        ps->state[1] = 4096;
        ps->state[2] = 4;
        ps->out = units * 2304;
        return true;
    case SYMACCEL_BATCH_FLAC_RESTORE:  // symaccel_flac_restore(_stereo_device): buf (in place), desc, coeffs [, pair_mode]; units = block size
        // frame.rs:58 (u16 block size); param = 0, or 0x100 | out_shift; the verify forms 0x200 | (nch - 1) << 12 and 0x300 | out_shift | (nch - 1) << 12
        if (units > 65535 || param < 0 || (param & ~((param & 0x200) ? 0x731f : 0x11f)) || ((param & 0x300) == 0x200 && (param & 31))) return false;
        ps->n_in = pair_param(param).pairs || flac_verify_param(param).verify ? 4 : 3;
        ps->in[0] = units * 4;
        ps->in[1] = sizeof(symaccel_flac_desc);
        ps->in[2] = 32 * 4;
        if (pair_param(param).pairs) {
            ps->in[3] = 1;
            ps->in_div[3] = 2;
        }
        if (flac_verify_param(param).verify) {  // a frame record and a state per FRAME: entry 0 in, every frame's checkpoint out
            ps->in[3] = sizeof(symaccel_flac_md5_frame);
            ps->in_div[3] = ps->state_div = (uint8_t)flac_verify_param(param).nch;
            ps->n_state = 1;
            ps->state[0] = sizeof(symaccel_md5_state);
        }
        ps->in_place = true;
        return true;
    case SYMACCEL_BATCH_ALAC_PREDICT:  // symaccel_alac_predict(_stereo_device): buf (in place), desc, coeffs [, pair_weight, pair_shift]
        if (units > 0x3fffffffu || (param & ~0x100)) return false;
        ps->n_in = pair_param(param).pairs ? 5 : 3;
        ps->in[0] = units * 4;
        ps->in[1] = sizeof(symaccel_alac_desc);
        ps->in[2] = 32 * 4;
        if (pair_param(param).pairs) {
            ps->in[3] = 4;
            ps->in_div[3] = 2;
            ps->in[4] = 1;
            ps->in_div[4] = 2;
        }
        ps->in_place = true;
        return true;
    case SYMACCEL_BATCH_ADPCM_DECODE: {  // symaccel_adpcm_decode: bytes | no state | pcm; a chain is a BLOCK, units = its bytes
        // param = codec | channels << 8 (| out_fmt << 16 inside the batcher: reserve_fmt folds the format into the group key, and the
        // kernel itself writes the interleaved samples -- the scatter copies them as they are)
        const AdpcmParam ap = adpcm_param(param);
        const size_t fpb = adpcm_frames_of_bytes(ap.codec, (size_t)ap.nch, units);
        if (param < 0 || (param >> 24) || fpb == 0 || (ap.fmt != 0 && symaccel_sample_bytes(ap.fmt) == 0)) return false;
        ps->n_in = 1;
        ps->in[0] = units;
        ps->out = (size_t)ap.nch * fpb * (ap.fmt ? symaccel_sample_bytes(ap.fmt) : 4);
        return true;
    }
    case SYMACCEL_BATCH_MPA12_DECODE: {  // symaccel_mpa12_decode: codes, rec | vvec, vfront | pcm; param = the layer
        const size_t nf = (size_t)mpa12_n_frames(param);
        if (nf == 0 || units > 0x3fffffffu) return false;
        ps->n_in = 2;
        ps->in[0] = units * 32 * nf * 2;
        ps->in[1] = units * symaccel_mpa12_record_bytes(param);
        ps->n_state = 2;
        ps->state[0] = 4096;
        ps->state[1] = 4;
        ps->out = units * 32 * nf * 4;
        return true;
    }
    case SYMACCEL_BATCH_PCM_DECODE: {  // symaccel_pcm_decode: bytes | no state | pcm; a chain is a PACKET, units = its frames
        // param = codec | channels << 8 | shift << 16 (| out_fmt << 24 inside the batcher, as for ADPCM_DECODE)
        const PcmDecParam pp = pcmdec_param(param);
        if (param < 0 || (param >> 28) || units > 0x3fffffffu) return false;
        if (pcm_decode_shape_status(kPcmDecMaxPitch, 1, pp.codec, (size_t)pp.nch, (unsigned)pp.shift, units, pp.fmt) != SYMACCEL_OK) return false;
        const PcmCodec pc = pcm_codec(pp.codec);
        ps->n_in = 1;
        ps->in[0] = units * (size_t)pp.nch * pc.coded;
        ps->out = units * (size_t)pp.nch * (pp.fmt ? symaccel_sample_bytes(pp.fmt) : pc.native);
        return true;
    }
    default: return false;
    }
}

// What a launch costs is not the same for every kind: the FLAC / ALAC kernels walk a block's recurrence with ONE lane (4096 samples at
// ~120 ns each: half a millisecond whatever the launch holds), so their groups are worth launching only when they are large -- four
// times the input of the transform kinds before a group goes unasked, and a hint launches nothing below `flush_bytes`
// (measured: 0.39 -> 0.74 M packets/s of 4096-sample stereo frames at 256 streams, profiles/r06k_decoders.jsonl).
inline bool serial_kind(int kind) { return kind == SYMACCEL_BATCH_FLAC_RESTORE || kind == SYMACCEL_BATCH_ALAC_PREDICT; }
inline size_t flush_threshold(size_t flush_bytes, int kind) { return serial_kind(kind) ? 4 * flush_bytes : flush_bytes; }
inline size_t hint_threshold(size_t hint_bytes, size_t flush_bytes, int kind) { return serial_kind(kind) ? std::max(hint_bytes, 2 * flush_bytes) : hint_bytes; }

inline size_t plane_bytes(const PlaneSizes &ps, int i, size_t n_chains) { return ps.in_per_ticket[i] ? ps.in[i] : ps.in[i] * (n_chains / ps.in_div[i]); }

size_t in_bytes_per_chain(const PlaneSizes &ps) {
    size_t s = 0;
    for (int i = 0; i < ps.n_in; ++i)
        if (!ps.in_per_ticket[i]) s += ps.in[i] / ps.in_div[i];
    return s;
}

SlotLayout slot_layout(const PlaneSizes &ps, size_t n_chains) {
    SlotLayout l;
    size_t off = 0;
    for (int i = 0; i < ps.n_in; ++i) {
        l.in[i] = off;
        l.in_bytes[i] = plane_bytes(ps, i, n_chains);
        off += round256(l.in_bytes[i]);
    }
    for (int i = 0; i < ps.n_state; ++i) {
        l.state[i] = off;
        l.state_bytes[i] = ps.state[i] * (n_chains / ps.state_div);
        off += round256(l.state_bytes[i]);
    }
    if (ps.in_place) {
        l.out = l.in[0];
        l.out_bytes = l.in_bytes[0];
    } else {
        l.out = off;
        l.out_bytes = ps.out * n_chains;
        off += round256(l.out_bytes);
    }
    l.bytes = off;
    return l;
}

// Slots are pooled by size CLASS, not by exact size: eight classes per octave (at most 12.5 % of padding), so the odd shapes of a
// running service -- tail batches at the end of a stream, short look-ahead batches, MP3 granule totals -- reuse each other's memory
// instead of each carving a slab of its own.
size_t slot_class(size_t bytes) {
    if (bytes <= 4096) return 4096;
    size_t top = (size_t)1 << (63 - __builtin_clzll((unsigned long long)bytes));
    const size_t step = top >> 3;
    return (bytes + step - 1) & ~(step - 1);
}

struct Group;
using Clock = std::chrono::steady_clock;

struct Ticket {
    Group *group = nullptr;
    uint32_t gen = 0;
    uint32_t first_chain = 0, n_chains = 0;
    bool live = false, committed = false;
    Clock::time_point committed_at{};
    int status = SYMACCEL_OK;  // of THIS submission, once its group is launched
    char *slot = nullptr;      // page-locked, slot_layout(group's planes, n_chains)
    size_t slot_bytes = 0;     // (the size class it was carved for)
    // copy form (symaccel_batcher_submit): where collect() puts the results
    void *user_state[kMaxState] = {nullptr, nullptr, nullptr};
    void *user_out = nullptr;
    // the output format asked for (symaccel_batcher_reserve_fmt; 0 = the native planes), the chains of an interleave group, and the bytes
    // of slot.out that are valid: the most the shape can give at reserve(), what the launch wrote afterwards
    int out_fmt = 0;
    uint32_t channels = 0;
    size_t out_valid = 0;
    // the input format (symaccel_batcher_reserve_io): 0 = the native planes, SYMACCEL_FMT_S16 = plane 0 of the slot holds int16_t words
    // -- the first half of the region the native plane (and the result, in place) has; SYMACCEL_IN_FMT_ROWS = every row of plane 0 at
    // its native offset, at a width of its own: the width table (slot.input[5], a byte per row) lies behind the shape's planes in the slot
    int in_fmt = 0;
};

enum class GroupState { Free, Open, Closed, Launching, Launched };

struct Lane;

// The device side of a launch: one allocation (cut into the planes of whatever group is launched with it), the page-locked copy
// descriptors and lists, the events of the chunk pipeline.  Blocks are POOLED apart from the groups: a group stays around until the
// last of its submissions is released -- the decoders hold their current batch for as long as they hand it out -- but the device
// memory is free again as soon as the scatter has finished, so a handful of blocks serve any number of groups in flight.
struct Block {
    char *d_base = nullptr;
    size_t d_bytes = 0;
    char *h_desc = nullptr;
    size_t h_desc_bytes = 0;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr};
    // completion: a word of page-locked memory the launch's last kernel writes its sequence number into (batch_flag_kernel); the
    // numbers of a block only grow, so "flag >= seq" stays true for a launch that has finished however often the block is reused
    uint64_t *h_flag = nullptr;
    uint64_t seq = 0;
    Group *owner = nullptr;  // the group whose launch is (or was last) using it; nullptr: never used or given back
};

inline uint64_t read_flag(const uint64_t *flag) { return __atomic_load_n(flag, __ATOMIC_ACQUIRE); }

// How a launch is cut and copied: development knobs, read once per batcher (symaccel_batcher_create)
struct LaunchKnobs {
    bool row_pad = true;                  // SYMACCEL_BATCH_ROW_PAD=0 keeps the rows of a FLAC / ALAC device plane back to back
    size_t dma_bytes = 0;                 // SYMACCEL_BATCH_DMA_KB: bulk planes of this size or more go through a copy engine (0 = none)
    size_t chunk_div = 2;                 // SYMACCEL_BATCH_CHUNKS: chunks a full group is cut into (1 .. 64)
    size_t chunk_min = (size_t)8192 << 10;  // SYMACCEL_BATCH_CHUNK_MIN_KB: the smallest chunk (at least 64 KiB)
};

// One launch: the submissions of one shape that were pending together.  Host side: the submissions' own slots.  Device side: a
// Block, cut at launch time (when the number of chains is known).
struct Group {
    int kind = 0, param = 0;
    size_t units = 0;
    PlaneSizes ps;
    size_t cap_chains = 0;  // reservations accepted before the group is launched and a fresh one opened
    size_t chains = 0, tickets = 0, uncommitted = 0, live = 0;
    Clock::time_point launched_at{};  // (enqueued: statistics)
    GroupState state = GroupState::Free;
    int status = SYMACCEL_OK;          // of the launch as a whole (a device error fails every ticket)
    std::vector<uint32_t> ticket_ids;  // the submissions, in order (index into symaccel_batcher::tickets)
    std::vector<TicketView> views;     // ... as the launch sees them
    Lane *lane = nullptr;              // where it was (is being) enqueued
    Block *block = nullptr;            // its device side, until somebody has seen the launch complete
    bool completed = false;            // its launch has been seen complete (or failed and was drained): nothing of it is in flight
    const uint64_t *done_flag = nullptr;  // where its launch reports completion, and the number that means "this launch"
    uint64_t done_seq = 0;
    char *d_in[kMaxIn] = {}, *d_state_in[kMaxState] = {}, *d_state_out[kMaxState] = {}, *d_out = nullptr;
    size_t row_pitch = 0;  // FLAC_RESTORE / ALAC_PREDICT: bytes between the chains (rows) of d_in[0] when the device plane is padded (symaccel_row_stride), 0 = rows back to back
    LaunchKnobs knobs;          // the batcher's (copied when the group closes)
    std::vector<VorbisUsed> used;  // the two Vorbis kinds: what every chain's blocks fill (TicketView::used points into it)
    Mp3Lists mp3;               // the lists of the kind the group is of (batcher_lists.h)
    AacLists aac;
    VorbisLists vb;
    FlacVerifyLists fv;
};

// One pipeline: a context (kernel stream, scratch, tables) and two copy streams.  Lane 0 is the caller's context; the others are the
// batcher's own.  `mu` serialises the enqueues of a lane (a context is externally synchronised).
struct Lane {
    symaccel_ctx *ctx = nullptr;
    bool owned = false;
    std::mutex mu;
};

inline uint64_t ns_since(Clock::time_point t0) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count(); }

}  // namespace

struct symaccel_batcher {
    symaccel_ctx *ctx = nullptr;
    size_t flush_bytes = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::unique_ptr<Group>> groups;
    std::vector<Ticket> tickets;
    std::vector<uint32_t> free_tickets;
    symaccel_batcher_stats stats{};
    std::string last_error;
    LaunchKnobs knobs;
    size_t hint_bytes = 0;  // what a group must hold for a hint to launch it ...
    size_t busy_groups = 4, busy_hint_bytes = (size_t)48 << 20;  // ... and while at least `busy_groups` launches are in flight
    std::vector<std::unique_ptr<Lane>> lanes;
    size_t want_lanes = 2, next_lane = 0;
    std::vector<std::unique_ptr<Block>> blocks;
    // page-locked slot memory: slabs, carved into slots by size class; a released slot goes to the free list of its class (the
    // shapes of a running service repeat: in the steady state nothing is allocated)
    struct Slab {
        char *base;
        size_t bytes, used;
    };
    std::vector<Slab> slabs;
    uint64_t slots_live = 0;
    bool growing = false;  // a caller is page-locking a new slab (outside the mutex): the others wait for it instead of adding their own
    std::vector<std::pair<size_t, std::vector<char *>>> free_slots;
    // AAC_DECODE: the scale-factor-band tables a stream's joint-stereo descriptors refer to, registered once per stream shape
    // (symaccel_batcher_aac_bands); a submission names its table by index (`param`), which is part of the group key
    struct Bands {
        std::vector<uint16_t> swb_long, swb_short;
        AacBandMaps maps;
    };
    std::vector<Bands> bands;
    // VORBIS_DECODE: the floor-1 configurations the submissions' floor planes index (symaccel_batcher_vorbis_floor)
    std::vector<symaccel_vorbis_floor1_cfg> floors;
};

namespace {

constexpr size_t kSlabBytes = (size_t)32 << 20;

// (the batcher's mutex, with the time spent waiting for it on the books: symaccel_batcher_stats::mutex_wait_ns)
struct Locked {
    std::unique_lock<std::mutex> lock;
    explicit Locked(symaccel_batcher *b) : lock(b->mu, std::defer_lock) {
        if (!lock.try_lock()) {
            const Clock::time_point t0 = Clock::now();
            lock.lock();
            b->stats.mutex_wait_ns += ns_since(t0);
            b->stats.mutex_contended += 1;
        }
    }
};

// mu held on entry and on return; DROPPED while a new slab is page-locked (hipHostMalloc of tens of MiB takes milliseconds: held, it
// stalled every other caller -- 1.1 to 1.6 s of summed mutex wait in a 0.4 s run, profiles/r06c_decoders.jsonl).  Slabs double in
// size up to 128 MiB, so a service that grows does so in a few steps.
int slot_alloc(symaccel_batcher *b, std::unique_lock<std::mutex> &lock, size_t bytes, char **out) {
    for (;;) {
        for (auto &cls : b->free_slots)
            if (cls.first == bytes && !cls.second.empty()) {
                *out = cls.second.back();
                cls.second.pop_back();
                return SYMACCEL_OK;
            }
        for (auto &sl : b->slabs)
            if (sl.bytes - sl.used >= bytes) {
                *out = sl.base + sl.used;
                sl.used += bytes;
                return SYMACCEL_OK;
            }
        if (b->growing) {  // somebody is page-locking a slab right now: its memory will do for this caller too
            b->cv.wait(lock, [&] { return !b->growing; });
            continue;
        }
        static const size_t slab0 = [] {  // (test knob: the first slab's size in KiB)
            const char *e = std::getenv("SYMACCEL_BATCHER_SLAB_KB");
            return e && std::atol(e) > 0 ? (size_t)std::atol(e) << 10 : kSlabBytes;
        }();
        size_t want = slab0;
        if (!b->slabs.empty()) want = std::min<size_t>(4 * slab0, 2 * b->slabs.back().bytes);
        want = std::max(want, bytes);
        void *h = nullptr;
        b->growing = true;
        lock.unlock();
        int st = SYMACCEL_OK;
        {
            DeviceGuard dev(b->ctx);
            if (!dev.ok()) st = dev.status();
            else if (hipHostMalloc(&h, want, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                st = SYMACCEL_ERR_OOM;
            }
        }
        lock.lock();
        b->growing = false;
        b->cv.notify_all();
        if (st != SYMACCEL_OK) return st;
        b->slabs.push_back({static_cast<char *>(h), want, 0});
        b->stats.staging_bytes += want;
    }
}

void slot_free(symaccel_batcher *b, char *p, size_t bytes) {
    if (!p) return;
    for (auto &cls : b->free_slots)
        if (cls.first == bytes) {
            cls.second.push_back(p);
            return;
        }
    b->free_slots.push_back({bytes, {p}});
}

void block_free(Block *k) {
    if (k->d_base) (void)hipFree(k->d_base);
    if (k->h_desc) (void)hipHostFree(k->h_desc);
    for (hipEvent_t e : {k->ev_in[0], k->ev_in[1], k->ev_k[0], k->ev_k[1]})
        if (e) (void)hipEventDestroy(e);
    if (k->h_flag) (void)hipHostFree(k->h_flag);
    k->h_flag = nullptr;
    k->d_base = nullptr;
    k->h_desc = nullptr;
}

inline bool vorbis_kind(int kind) { return kind == SYMACCEL_BATCH_VORBIS_SYNTH || kind == SYMACCEL_BATCH_VORBIS_DECODE; }

// ---- what a FLAC / ALAC / ADPCM submission's descriptors say, judged alone (its neighbours in the launch are not failed for it; the
// kinds that have lists judge theirs in batcher_lists.h); then the steps of a launch (launch_group_inner) in their order
// a ticket with a width per row (SYMACCEL_IN_FMT_ROWS): every byte of its width table is 2, 3 or 4
bool row_widths_ok(const TicketView &v) {
    if (v.in_fmt != SYMACCEL_IN_FMT_ROWS) return true;
    const uint8_t *w = v.row_bytes();
    for (size_t c = 0; c < v.n_chains; ++c)
        if (w[c] < 2 || w[c] > 4) return false;
    return true;
}

int check_flac(size_t units, int param, const TicketView &v) {
    if (!row_widths_ok(v)) return SYMACCEL_ERR_INVALID_ARG;
    const FlacVerifyParam vp = flac_verify_param(param);
    if (vp.verify) {  // the frame records, as flac_md5_kernel judges a job -- and every frame names its width
        const symaccel_flac_md5_frame *fr = v.in<const symaccel_flac_md5_frame>(3);
        for (size_t f = 0; f < v.n_chains / vp.nch; ++f)
            if (fr[f].block_len > units || fr[f].pair_mode > 3 || (fr[f].pair_mode != 0 && vp.nch != 2) || fr[f].bytes_per_sample < 1 || fr[f].bytes_per_sample > 4)
                return SYMACCEL_ERR_INVALID_ARG;
    }
    const symaccel_flac_desc *d = v.in<const symaccel_flac_desc>(1);
    for (size_t c = 0; c < v.n_chains; ++c) {  // what symaccel_flac_restore checks (decoder.rs:361, 456-458, 506-508)
        if (d[c].kind > SYMACCEL_FLAC_LPC || d[c].order > units || d[c].shift > 31 || d[c].wasted_bits > 31) return SYMACCEL_ERR_INVALID_ARG;
        if (d[c].kind == SYMACCEL_FLAC_FIXED && d[c].order > 4) return SYMACCEL_ERR_INVALID_ARG;
        if (d[c].kind == SYMACCEL_FLAC_LPC && (d[c].order < 1 || d[c].order > 32)) return SYMACCEL_ERR_INVALID_ARG;
    }
    if (pair_param(param).pairs) {
        const uint8_t *pm = v.in<const uint8_t>(3);
        for (size_t p = 0; p < v.n_chains / 2; ++p)
            if (pm[p] > 3) return SYMACCEL_ERR_INVALID_ARG;
    }
    return SYMACCEL_OK;
}

int check_alac(int param, const TicketView &v) {
    if (!row_widths_ok(v)) return SYMACCEL_ERR_INVALID_ARG;
    const symaccel_alac_desc *d = v.in<const symaccel_alac_desc>(1);
    for (size_t c = 0; c < v.n_chains; ++c) {
        if (d[c].mode > 0 && d[c].mode < 15) return SYMACCEL_ERR_DECODE;  // lib.rs:167-169, "alac: invalid mode" (symaccel_alac_block_status_device)
        if (d[c].lpc_order > 31 || d[c].shift > 31 || d[c].bps < 1 || d[c].bps > 32) return SYMACCEL_ERR_INVALID_ARG;
    }
    if (pair_param(param).pairs) {
        const uint8_t *sh = v.in<const uint8_t>(4);
        for (size_t p = 0; p < v.n_chains / 2; ++p)
            if (sh[p] > 31) return SYMACCEL_ERR_INVALID_ARG;  // lib.rs:555
    }
    return SYMACCEL_OK;
}

// An ADPCM_DECODE submission: the status its first rejected block has (symaccel_adpcm_decode_device's per-block status, read from the
// preambles here: the reference stops a packet at its first bad block -- codec_ms.rs:25-29 Unsupported, codec_ima_wav.rs:17-19 DecodeError)
int check_adpcm(size_t units, int param, const TicketView &v) {
    const AdpcmParam ap = adpcm_param(param);
    const uint8_t *b = v.in<const uint8_t>(0);
    for (size_t c = 0; c < v.n_chains; ++c, b += units)
        for (int k = 0; k < ap.nch; ++k) {
            if (ap.codec == SYMACCEL_ADPCM_MS && b[k] > 6) return SYMACCEL_ERR_UNSUPPORTED;
            if (ap.codec == SYMACCEL_ADPCM_IMA_WAV && b[4 * k + 2] > 88) return SYMACCEL_ERR_DECODE;
        }
    return SYMACCEL_OK;
}

// An MPA12_DECODE submission: SYMACCEL_ERR_INVALID_ARG if any of its records is one the kernel marks with status 1 (Mpa12Lane::out_of_range,
// csrc/mpa12_dequant.h: Layer I bits of 1 or above 15, a class above 17, a scale-factor index above 63).  Such a submission runs as
// silence: its records are cleared in the slot, so every channel-packet of it allocates nothing and the filterbank alone advances.
int check_mpa12(size_t units, int param, TicketView &v) {
    const size_t rb = symaccel_mpa12_record_bytes(param);
    uint8_t *r = v.in<uint8_t>(1);
    bool bad = false;
    for (size_t k = 0; k < v.n_chains * units && !bad; ++k, r += rb)
        for (size_t i = 0; i < rb && !bad; ++i)
            bad = i >= 32 ? r[i] > 63 : (param == SYMACCEL_MPA_LAYER1 ? r[i] == 1 || r[i] > 15 : r[i] > (uint8_t)kMpa12Classes);
    if (!bad) return SYMACCEL_OK;
    std::memset(v.slot + v.lay.in[1], 0, v.lay.in_bytes[1]);
    return SYMACCEL_ERR_INVALID_ARG;
}

// Per-ticket facts, computed once in front of the first chunk: the slot's layout; Vorbis: what every chain's flags account for (the
// state planes they depend on are overwritten by the scatter of the ticket's chunk -- gather, scatter and out_valid all read these).
// Submissions with an output format (symaccel_batcher_reserve_fmt) leave as converting pieces, a frame range of one interleave group
// each: the bytes that will be valid, and a submission whose chains of one interleave group disagree fails alone.
void prepare_views(Group *g) {
    const PlaneSizes &ps = g->ps;
    const VorbisParam vp = vorbis_param(g->param, g->units);
    if (vorbis_kind(g->kind)) g->used.resize(g->chains);
    for (TicketView &v : g->views) {
        v.lay = slot_layout(ps, v.n_chains);
        if (vorbis_kind(g->kind)) {
            VorbisUsed *used = g->used.data() + v.first_chain;
            for (size_t c = 0; c < v.n_chains; ++c) used[c] = vorbis_used(v.in<const uint8_t>(1) + c * g->units, g->units, v.state<const int32_t>(0)[c], vp.e0, vp.e1);
            v.used = used;
        }
        if (!v.out_fmt) continue;
        const size_t fb = (size_t)v.channels * symaccel_sample_bytes(v.out_fmt);
        v.out_valid = (v.n_chains / v.channels) * (ps.out_per_chain() / 4) * fb;
        if (!vorbis_kind(g->kind)) continue;
        v.out_valid = 0;
        for (size_t c = 0; c < v.n_chains; ++c) {
            if (c % v.channels == 0) v.out_valid += v.used[c].samples * fb;
            else if (v.used[c].samples != v.used[c - c % v.channels].samples) v.fmt_status = SYMACCEL_ERR_INVALID_ARG;
        }
        // like every other per-ticket failure it runs as an empty description: silence in (VORBIS_DECODE: no floors and no steps either,
        // through its status), nothing of the stream's data reaches the kernels, and no PCM comes back
        if (v.fmt_status != SYMACCEL_OK) std::memset(v.slot + v.lay.in[0], 0, v.lay.in_bytes[0]);
    }
}

// The submissions' own descriptors, each judged alone: one that does not add up is neutralised (it runs as an empty description, its
// ticket fails) and the rest of the launch goes ahead.  The kinds with lists count them on the way.
void validate_and_count(Group *g) {
    if (g->kind == SYMACCEL_BATCH_AAC_DECODE) g->aac.count(g->views, g->ps, g->units, g->param);
    if (g->kind == SYMACCEL_BATCH_VORBIS_DECODE) g->vb.count(g->views, g->ps, g->units, g->chains);
    for (TicketView &v : g->views) {
        if (g->kind == SYMACCEL_BATCH_FLAC_RESTORE) v.status = check_flac(g->units, g->param, v);
        if (g->kind == SYMACCEL_BATCH_ALAC_PREDICT) v.status = check_alac(g->param, v);
        if (g->kind == SYMACCEL_BATCH_ADPCM_DECODE) v.status = check_adpcm(g->units, g->param, v);
        if (g->kind == SYMACCEL_BATCH_MPA12_DECODE) v.status = check_mpa12(g->units, g->param, v);
        if (v.status == SYMACCEL_OK) v.status = v.fmt_status;
        // a verify submission that failed is not hashed (its job has no state: FlacVerifyLists::build), and its state plane is not
        // brought back: every entry is its starting state from here on
        if (g->kind == SYMACCEL_BATCH_FLAC_RESTORE && flac_verify_param(g->param).verify && v.status != SYMACCEL_OK) {
            symaccel_md5_state *st = v.state<symaccel_md5_state>(0);
            for (size_t f = 1; f < v.n_chains / g->ps.state_div; ++f) st[f] = st[0];
        }
    }
    // FLAC / ALAC: the device plane's rows at the pitch the lane-per-block kernels run fastest at (symaccel_row_stride: rows 4 / 8 / 16 / 32 KiB apart -- the
    // 4096-sample blocks of nearly every stream -- put a wavefront's 64 row segments on a fraction of the HBM channels); the slots stay compact, the
    // gather / scatter go row by row
    g->row_pitch = serial_kind(g->kind) && g->knobs.row_pad && symaccel_row_stride(g->units) * 4 != g->ps.in[0] ? symaccel_row_stride(g->units) * 4 : 0;
}

// An upper bound of the copy pieces of the launch, gathers and scatters of every chunk together: what the descriptor area is sized
// for (Pieces refuses to write beyond it)
size_t piece_bound(const Group *g) {
    const PlaneSizes &ps = g->ps;
    size_t bound = 0;
    for (const TicketView &v : g->views) {
        for (int i = 0; i < ps.n_in; ++i)
            if (!ps.in_host_only[i]) bound += pieces_of(plane_bytes(ps, i, v.n_chains));         // every plane that is copied, rounded up
        for (int i = 0; i < ps.n_state; ++i) bound += 2 * pieces_of(ps.state[i] * (v.n_chains / ps.state_div));  // the state, in and out
        bound += pieces_of(ps.out_per_chain() * v.n_chains);                                     // the PCM
        if (v.out_fmt) {  // ... or its converting pieces: a tile of frames each, the last of every interleave group rounded up
            const size_t tile = pcm_tile_frames(v.channels, (unsigned)symaccel_sample_bytes(v.out_fmt));
            bound += (v.n_chains / v.channels) * ((ps.out_per_chain() / 4 + tile - 1) / tile + 1);
        }
        if (g->kind == SYMACCEL_BATCH_AAC_DECODE) bound += pieces_of(ps.in[2] * v.n_chains);  // the joint-stereo rows of the blob
    }
    bound += g->tickets + 8;                                // the unit list's pieces, one per chunk at most
    if (g->kind == SYMACCEL_BATCH_FLAC_RESTORE && flac_verify_param(g->param).verify) bound += 2 * g->tickets + 8;  // the job table's, likewise
    if (g->row_pitch) bound += 2 * g->chains;               // rows go one by one, in and out, each rounded up
    for (const TicketView &v : g->views)
        if (v.in_fmt == SYMACCEL_IN_FMT_ROWS) bound += v.n_chains;  // ... and the rows of a ticket with a width per row go in one by one always
    if (vorbis_kind(g->kind)) bound += 2 * g->chains;       // spectra and PCM go chain by chain, each rounded up
    if (g->kind == SYMACCEL_BATCH_AAC_DECODE) bound += 3 * g->tickets + 8;  // pair list, filters, TNS pair frames: one piece list each per chunk
    if (g->kind == SYMACCEL_BATCH_VORBIS_DECODE) {          // its six lists: cut once per chunk, each cut rounded up
        const auto &b = g->vb.bytes;
        bound += 6 * (g->tickets + 8) + pieces_of(b.boff) + pieces_of(b.kill) + pieces_of(b.first) + pieces_of(b.steps) + pieces_of(b.ys) + pieces_of(b.offs);
    }
    return bound;
}

// `bytes` of a block's device or page-locked memory: grown, never shrunk.  (hipFree waits for the whole device, hipMalloc is not
// cheap either: a group's memory is sized for what the group can hold at most -- cap_chains, i.e. flush_bytes of input -- the first
// time, so that groups of fewer submissions never have to grow later; measured before: 0.87 ms of host time per launch with four
// caller threads, profiles/r06b_decoders.jsonl)
size_t grown(const Group *g, size_t bytes, size_t slack) {
    return std::max(bytes + bytes / 4, (bytes / std::max<size_t>(1, g->chains) + 1) * std::max(g->cap_chains, g->chains) + slack);
}

// What a closed group needs of its block, every plane and list requested once: device memory (`dev`) and the page-locked area
// (`host`: [copy descriptors | the lists the host builds])
void request_block(Group *g, size_t bound, BatchCopyDesc **descs, Carver &dev, Carver &host) {
    const PlaneSizes &ps = g->ps;
    host.want(descs, bound * sizeof(BatchCopyDesc));
    for (int i = 0; i < ps.n_in; ++i) {
        g->d_in[i] = nullptr;
        if (ps.in_host_only[i]) continue;
        dev.want(&g->d_in[i], ps.in_per_ticket[i] ? ps.in[i] * g->tickets : (i == 0 && g->row_pitch ? g->row_pitch : ps.in[i]) * ((g->chains + ps.in_div[i] - 1) / ps.in_div[i]));
    }
    for (int i = 0; i < ps.n_state; ++i) {
        dev.want(&g->d_state_in[i], ps.state[i] * (g->chains / ps.state_div));
        dev.want(&g->d_state_out[i], ps.state[i] * (g->chains / ps.state_div));
    }
    if (ps.in_place) g->d_out = g->d_in[0];
    else dev.want(&g->d_out, ps.out * g->chains);
    g->mp3.request(dev, host, g->tickets);  // (by every kind: the blocks keep the sizes -- and the statistics their group_allocs -- they had)
    if (g->kind == SYMACCEL_BATCH_AAC_DECODE) g->aac.request(dev, host, g->chains, g->units);
    if (g->kind == SYMACCEL_BATCH_FLAC_RESTORE && flac_verify_param(g->param).verify) g->fv.request(dev, host, g->tickets);
    if (g->kind == SYMACCEL_BATCH_VORBIS_DECODE) g->vb.request(dev, host, g->chains, vorbis_param(g->param, g->units).cap);
}

// the device side of a closed group: its block grown to what the group needs (carved without memory), then carved
int carve_block(symaccel_ctx *ctx, Group *g, size_t bound, BatchCopyDesc **descs, uint64_t *n_allocs) {
    Block *blk = g->block;
    Carver dev, host;
    request_block(g, bound, descs, dev, host);
    if (dev.total > blk->d_bytes) {
        if (blk->d_base) SYM_GPU(ctx, hipFree(blk->d_base));
        blk->d_base = nullptr;
        blk->d_bytes = 0;
        void *d = nullptr;
        const size_t want = grown(g, dev.total, (size_t)1 << 20);
        SYM_TRY(ctx_alloc(ctx, &d, want, false));
        blk->d_base = static_cast<char *>(d);
        blk->d_bytes = want;
        *n_allocs += 1;
    }
    if (host.total > blk->h_desc_bytes) {
        if (blk->h_desc) (void)hipHostFree(blk->h_desc);
        blk->h_desc = nullptr;
        blk->h_desc_bytes = 0;
        void *h = nullptr;
        const size_t want = grown(g, host.total, 65536);
        if (hipHostMalloc(&h, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return SYMACCEL_ERR_OOM;
        }
        blk->h_desc = static_cast<char *>(h);
        blk->h_desc_bytes = want;
        *n_allocs += 1;
    }
    Carver dev_mem{blk->d_base}, host_mem{blk->h_desc};
    request_block(g, bound, descs, dev_mem, host_mem);
    for (hipEvent_t *e : {&blk->ev_in[0], &blk->ev_in[1], &blk->ev_k[0], &blk->ev_k[1]})
        if (!*e) SYM_GPU(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return SYMACCEL_OK;
}

// The chunk that starts at submission t0.  Half of the group per chunk, 8 .. 32 MiB of input: a chunk costs three launches and two
// event hops (~40 us), which 2 MiB chunks (44 us on the link) did not amortise -- 22.7 GB/s each way at look-ahead 64 against 37.9 at
// 256 (profiles/r05c_*); consecutive GROUPS overlap on the lanes anyway, so a small group is one chunk (one or two chunks measure the
// same, three or six are slower: profiles/r06z4_big_groups.jsonl, r06z5_copy_grid.jsonl)
Chunk next_chunk(const Group *g, size_t t0) {
    const PlaneSizes &ps = g->ps;
    const size_t per_chain = std::max<size_t>(1, in_bytes_per_chain(ps));
    const size_t chunk_bytes = std::min<size_t>((size_t)32 << 20, std::max<size_t>(g->knobs.chunk_min, g->chains * per_chain / g->knobs.chunk_div));
    const size_t chunk_chains = std::max<size_t>(1, chunk_bytes / per_chain);
    Chunk ch{};
    ch.c0 = g->views[t0].first_chain;
    ch.t0 = t0;
    size_t t1 = t0;
    while (t1 < g->tickets && (ch.nc == 0 || ch.nc + g->views[t1].n_chains <= chunk_chains)) ch.nc += g->views[t1++].n_chains;
    ch.nt = t1 - t0;
    for (int i = 0; i < ps.n_in; ++i)
        if (g->d_in[i]) ch.in[i] = g->d_in[i] + (ps.in_per_ticket[i] ? t0 * ps.in[i] : (ch.c0 / ps.in_div[i]) * (i == 0 && g->row_pitch ? g->row_pitch : ps.in[i]));
    for (int i = 0; i < ps.n_state; ++i) {
        ch.si[i] = g->d_state_in[i] + ch.c0 / ps.state_div * ps.state[i];
        ch.so[i] = g->d_state_out[i] + ch.c0 / ps.state_div * ps.state[i];
    }
    ch.out = ps.in_place ? ch.in[0] : g->d_out + ch.c0 * ps.out;
    return ch;
}

// the packed spectrum of a Vorbis submission: what the chain's blocks fill, not the plane
void gather_vorbis_spectra(const Group *g, const TicketView &t, Pieces &pw) {
    for (size_t c = 0; c < t.n_chains; ++c)
        pw.bulk(t.slot + t.lay.in[0] + c * g->ps.in[0], g->d_in[0] + ((size_t)t.first_chain + c) * g->ps.in[0], t.used[c].lines * 4);
}
// FLAC / ALAC: compact rows of the slot -> padded rows of the device plane
void gather_rows(const Group *g, const TicketView &t, Pieces &pw) {
    for (size_t c = 0; c < t.n_chains; ++c) pw.bulk(t.slot + t.lay.in[0] + c * g->ps.in[0], g->d_in[0] + ((size_t)t.first_chain + c) * g->row_pitch, g->ps.in[0]);
}

// FLAC / ALAC, a submission whose plane 0 came as int16_t (symaccel_batcher_reserve_io): widening pieces, row by row where the device
// plane is padded, the whole plane in one run where its rows are back to back
void gather_narrow(const Group *g, const TicketView &t, Pieces &pw) {
    const size_t row = g->ps.in[0];  // (the destination's bytes; the slot's rows are half of it)
    const char *src = t.slot + t.lay.in[0];
    if (!g->row_pitch) return pw.widen(src, g->d_in[0] + (size_t)t.first_chain * row, row * t.n_chains);
    for (size_t c = 0; c < t.n_chains; ++c) pw.widen(src + c * (row / 2), g->d_in[0] + ((size_t)t.first_chain + c) * g->row_pitch, row);
}

// FLAC / ALAC, a submission with a width per row (SYMACCEL_IN_FMT_ROWS): row by row always, every row from its native offset in the slot --
// a widening piece list at 2 or 3 bytes a word, plain pieces at 4 (and for a width that check_flac / check_alac refused: the ticket has
// failed, and the row's region is the native row's, so nothing outside the slot is read).  True if a widening piece was written.
bool gather_row_widths(const Group *g, const TicketView &t, Pieces &pw) {
    const size_t row = g->ps.in[0], pitch = g->row_pitch ? g->row_pitch : row;
    const uint8_t *w = t.row_bytes();
    bool widening = false;
    for (size_t c = 0; c < t.n_chains; ++c) {
        const char *src = t.slot + t.lay.in[0] + c * row;
        char *dst = g->d_in[0] + ((size_t)t.first_chain + c) * pitch;
        if (w[c] == 2 || w[c] == 3) pw.widen(src, dst, row, w[c]), widening = true;
        else pw.add(src, dst, row);
    }
    return widening;
}

// gather: the submissions' planes into the chain-major device arrays, and the chunk's lists; true if the list holds widening pieces
bool build_gather(Group *g, const Chunk &ch, Pieces &pw) {
    bool widening = false;
    const PlaneSizes &ps = g->ps;
    const bool verify = g->kind == SYMACCEL_BATCH_FLAC_RESTORE && flac_verify_param(g->param).verify;
    for (size_t ti = ch.t0; ti < ch.t0 + ch.nt; ++ti) {
        const TicketView &t = g->views[ti];
        for (int i = 0; i < ps.n_in; ++i) {
            if (ps.in_host_only[i]) continue;
            if (i == 0 && t.in_fmt == SYMACCEL_IN_FMT_ROWS) widening |= gather_row_widths(g, t, pw);
            else if (i == 0 && t.in_fmt) gather_narrow(g, t, pw), widening = true;
            else if (i == 0 && vorbis_kind(g->kind)) gather_vorbis_spectra(g, t, pw);
            else if (i == 0 && g->row_pitch) gather_rows(g, t, pw);
            else pw.bulk(t.slot + t.lay.in[i], g->d_in[i] + (ps.in_per_ticket[i] ? ti : (size_t)t.first_chain / ps.in_div[i]) * ps.in[i], t.lay.in_bytes[i]);
        }
        // (the verify forms of FLAC_RESTORE read entry 0 of a submission's state plane alone, its starting state: only that goes up)
        for (int i = 0; i < ps.n_state; ++i) pw.add(t.slot + t.lay.state[i], g->d_state_in[i] + (size_t)t.first_chain / ps.state_div * ps.state[i], verify ? ps.state[i] : t.lay.state_bytes[i]);
    }
    if (verify)
        g->fv.build(g->views, ch, flac_verify_param(g->param).nch, g->d_in[0], g->row_pitch ? g->row_pitch : ps.in[0], g->d_in[3], g->d_state_in[0], g->d_state_out[0], pw);
    if (g->kind == SYMACCEL_BATCH_MP3_DECODE) g->mp3.build(g->views, ch, pw);
    if (g->kind == SYMACCEL_BATCH_AAC_DECODE) g->aac.build(g->views, ch, g->units, pw);
    if (g->kind == SYMACCEL_BATCH_VORBIS_DECODE) g->vb.build(g->views, ch, vorbis_param(g->param, g->units), g->units, pw);
    return widening;
}

// The verify forms of FLAC_RESTORE: the unfused restore at the group's row pitch, then ONE MD5 launch over the chunk's submissions, a
// wavefront each (FINISH: it also leaves the planes decorrelated and left-justified).  Both on the lane's stream: the chain of this
// group (~1 us per 64-byte block per stream) overlaps the copies and the restore of the next group on another lane.
int launch_flac_verify(symaccel_ctx *ctx, Group *g, const Chunk &ch) {
    const FlacVerifyParam vp = flac_verify_param(g->param);
    SYM_TRY(launch_flac_restore(ctx, (int32_t *)ch.in[0], (const symaccel_flac_desc *)ch.in[1], (const int32_t *)ch.in[2], ch.nc, g->units, nullptr, 0, g->row_pitch / 4));
    return g->fv.run(ctx, ch, vp.finish, vp.shift);
}

// the kernels of one chunk
int launch_chunk(symaccel_ctx *ctx, Group *g, const Chunk &ch) {
    char *const *in = ch.in, *const *si = ch.si, *const *so = ch.so;
    switch (g->kind) {
    case SYMACCEL_BATCH_AAC_SYNTH:
        return launch_aac(ctx, (const float *)in[0], (const uint8_t *)in[1], (const float *)si[0], (float *)so[0], (float *)ch.out, ch.nc, g->units);
    case SYMACCEL_BATCH_MP3_SYNTH:
        return launch_mp3(ctx, (const float *)in[0], (const symaccel_mp3_side *)in[1], g->param, (const float *)si[0], (const float *)si[1],
                          (const int32_t *)si[2], (float *)so[0], (float *)so[1], (int32_t *)so[2], (float *)ch.out, ch.nc, g->units);
    case SYMACCEL_BATCH_MP3_DECODE: return g->mp3.run(ctx, ch, g->param, g->units);
    case SYMACCEL_BATCH_AAC_DECODE: return g->aac.run(ctx, ch, g->units);
    case SYMACCEL_BATCH_VORBIS_SYNTH: {
        const VorbisParam vp = vorbis_param(g->param, g->units);
        return symaccel_vorbis_synth_pp_device(ctx, vp.e0, vp.e1, (const float *)in[0], nullptr, vp.cap, (const uint8_t *)in[1], (const int32_t *)si[0],
                                               (int32_t *)so[0], (const float *)si[1], (float *)so[1], (float *)ch.out, vp.cap, ch.nc, g->units);
    }
    case SYMACCEL_BATCH_VORBIS_DECODE: return g->vb.run(ctx, ch, vorbis_param(g->param, g->units), g->units);
    case SYMACCEL_BATCH_FLAC_RESTORE: {  // decoder.rs:663-752 (+ :32-82, :239-242 with the pair modes)
        const PairParam pp = pair_param(g->param);
        if (flac_verify_param(g->param).verify) return launch_flac_verify(ctx, g, ch);
        return launch_flac_restore(ctx, (int32_t *)in[0], (const symaccel_flac_desc *)in[1], (const int32_t *)in[2], ch.nc, g->units,
                                   pp.pairs ? (const uint8_t *)in[3] : nullptr, pp.shift, g->row_pitch / 4);
    }
    case SYMACCEL_BATCH_ALAC_PREDICT: {  // alac/lib.rs:165-264 (+ :664-671 with the pair parameters)
        const bool pairs = pair_param(g->param).pairs;
        return launch_alac_predict(ctx, (int32_t *)in[0], (const symaccel_alac_desc *)in[1], (const int32_t *)in[2], ch.nc, g->units,
                                   pairs ? (const int32_t *)in[3] : nullptr, pairs ? (const uint8_t *)in[4] : nullptr, g->row_pitch / 4);
    }
    case SYMACCEL_BATCH_ADPCM_DECODE: {  // symphonia-codec-adpcm lib.rs:122-168 (the blocks of every packet in the chunk, side by side)
        const AdpcmParam ap = adpcm_param(g->param);
        return launch_adpcm_decode(ctx, ctx->stream, in[0], g->units, ch.nc, ap.codec, (unsigned)ap.nch,
                                   (unsigned)adpcm_frames_of_bytes(ap.codec, (size_t)ap.nch, g->units), ch.out, ap.fmt, nullptr);
    }
    case SYMACCEL_BATCH_PCM_DECODE: {  // symphonia-codec-pcm lib.rs:318-411 (the packets of the chunk, back to back)
        const PcmDecParam pp = pcmdec_param(g->param);
        return launch_pcm_decode(ctx, ctx->stream, in[0], g->ps.in[0], ch.nc, pp.codec, (unsigned)pp.nch, (unsigned)pp.shift, g->units, ch.out, pp.fmt);
    }
    case SYMACCEL_BATCH_MPA12_DECODE:  // layer1/mod.rs:142-194, layer2/mod.rs:320-384 (no status plane: check_mpa12 judged the records)
        return launch_mpa12_decode(ctx, g->param, (const uint16_t *)in[0], (const uint8_t *)in[1], nullptr, (const float *)si[0], (const int32_t *)si[1],
                                   (float *)so[0], (int32_t *)so[1], (float *)ch.out, ch.nc, g->units);
    default: return SYMACCEL_ERR_INVALID_ARG;
    }
}

// A submission with an output format: converted and interleaved on the way out, one piece per frame range of an interleave group, the
// groups packed behind each other at the front of slot.out (a submission that failed gets no PCM: nothing of it is valid)
bool scatter_converted(const Group *g, const TicketView &t, size_t plane_pitch, Pieces &pw) {
    const unsigned tile = pcm_tile_frames(t.channels, (unsigned)symaccel_sample_bytes(t.out_fmt));
    const size_t fb = (size_t)t.channels * symaccel_sample_bytes(t.out_fmt);
    char *dst = t.slot + t.lay.out;
    for (size_t c = 0; t.status == SYMACCEL_OK && c < t.n_chains; c += t.channels) {
        const size_t samples = t.used ? t.used[c].samples : g->ps.out_per_chain() / 4;
        const char *src = g->d_out + ((size_t)t.first_chain + c) * plane_pitch;
        for (size_t f0 = 0; f0 < samples; f0 += tile) {
            const size_t nf = std::min<size_t>(tile, samples - f0);
            pw.piece(src + f0 * 4, dst + f0 * fb, nf * fb, batch_piece_convert(serial_kind(g->kind), nf, t.channels, t.out_fmt));
        }
        dst += samples * fb;
    }
    return t.status == SYMACCEL_OK && t.n_chains != 0;
}

// scatter: PCM and the state after the batch back into the submissions' slots; *pcm_stride = the samples between the planes of d_out
// if there are converting pieces, else 0
void build_scatter(const Group *g, const Chunk &ch, Pieces &pw, size_t *pcm_stride) {
    const PlaneSizes &ps = g->ps;
    const size_t plane_pitch = g->row_pitch ? g->row_pitch : ps.out_per_chain();  // bytes between the chains of d_out
    const bool verify = g->kind == SYMACCEL_BATCH_FLAC_RESTORE && flac_verify_param(g->param).verify;
    bool converting = false;
    for (size_t ti = ch.t0; ti < ch.t0 + ch.nt; ++ti) {
        const TicketView &t = g->views[ti];
        if (t.out_fmt) {
            converting |= scatter_converted(g, t, plane_pitch, pw);
        } else if (vorbis_kind(g->kind)) {  // the packed PCM: what the chain's blocks yield, not the plane
            for (size_t c = 0; c < t.n_chains; ++c) pw.bulk(g->d_out + ((size_t)t.first_chain + c) * ps.out, t.slot + t.lay.out + c * ps.out, t.used[c].samples * 4);
        } else if (g->row_pitch) {  // (in place: d_out is d_in[0], padded rows)
            for (size_t c = 0; c < t.n_chains; ++c) pw.bulk(g->d_out + ((size_t)t.first_chain + c) * g->row_pitch, t.slot + t.lay.out + c * ps.in[0], ps.in[0]);
        } else {
            pw.bulk(g->d_out + (size_t)t.first_chain * plane_pitch, t.slot + t.lay.out, t.lay.out_bytes);
        }
        if (verify && t.status != SYMACCEL_OK) continue;  // (a verify submission that failed was not hashed: validate_and_count left its states in the slot)
        for (int i = 0; i < ps.n_state; ++i) pw.add(g->d_state_out[i] + (size_t)t.first_chain / ps.state_div * ps.state[i], t.slot + t.lay.state[i], t.lay.state_bytes[i]);
    }
    *pcm_stride = converting ? plane_pitch / 4 : 0;
}

// the pieces [first, pw.w) as ONE copy launch on `s`, the bulk planes that go through a copy engine in front of it
int enqueue_copies(symaccel_ctx *ctx, hipStream_t s, Pieces &pw, const BatchCopyDesc *first, bool scatter, size_t pcm_stride, bool widening = false) {
    if (pw.overflow) {  // (cannot happen while piece_bound() counts every contributor; nothing was written beyond the area)
        ctx->last_error = "batcher: a launch needs more copy pieces than piece_bound() counted";
        return SYMACCEL_ERR_DEVICE;
    }
    for (const Pieces::Dma &m : pw.dma) SYM_GPU(ctx, hipMemcpyAsync(m.dst, m.src, m.bytes, scatter ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, s));
    pw.dma.clear();
    return launch_batch_copy(ctx, s, first, (size_t)(pw.w - first), scatter, pcm_stride, widening);
}

// Everything of a closed group: per chunk of submissions ONE gather launch (slots -> HBM, the kernels' chain-major layout), the
// synthesis kernel(s), ONE scatter launch (HBM -> slots); `done` is recorded behind the last scatter.  Runs on `lane`, outside the
// batcher's mutex: nothing of the batcher but the group itself (and the slots its views point at) is touched.
int launch_group_inner(Lane *lane, Group *g, uint64_t *n_chunks, uint64_t *api_ns, uint64_t *n_allocs) {
    symaccel_ctx *ctx = lane->ctx;
    if (!ctx->stage_in) SYM_GPU(ctx, hipStreamCreate(&ctx->stage_in));
    if (!ctx->stage_out) SYM_GPU(ctx, hipStreamCreate(&ctx->stage_out));
    prepare_views(g);
    validate_and_count(g);
    const size_t bound = piece_bound(g);
    BatchCopyDesc *descs = nullptr;
    SYM_TRY(carve_block(ctx, g, bound, &descs, n_allocs));
    Block *blk = g->block;
    Pieces pw{descs, descs + bound, g->knobs.dma_bytes};
    for (size_t t0 = 0, k = 0; t0 < g->tickets; ++k) {
        const Chunk ch = next_chunk(g, t0);
        const int e = (int)(k & 1);
        const BatchCopyDesc *g0 = pw.w;
        const bool widening = build_gather(g, ch, pw);
        const Clock::time_point api0 = Clock::now();
        SYM_TRY(enqueue_copies(ctx, ctx->stage_in, pw, g0, false, 0, widening));
        SYM_GPU(ctx, hipEventRecord(blk->ev_in[e], ctx->stage_in));
        SYM_GPU(ctx, hipStreamWaitEvent(ctx->stream, blk->ev_in[e], 0));
        SYM_TRY(launch_chunk(ctx, g, ch));
        SYM_GPU(ctx, hipEventRecord(blk->ev_k[e], ctx->stream));
        SYM_GPU(ctx, hipStreamWaitEvent(ctx->stage_out, blk->ev_k[e], 0));
        *api_ns += ns_since(api0);
        const BatchCopyDesc *s0 = pw.w;
        size_t pcm_stride = 0;
        build_scatter(g, ch, pw, &pcm_stride);
        const Clock::time_point api1 = Clock::now();
        SYM_TRY(enqueue_copies(ctx, ctx->stage_out, pw, s0, true, pcm_stride));
        *api_ns += ns_since(api1);
        *n_chunks += 1;
        t0 += ch.nt;
    }
    return SYMACCEL_OK;
}

// the device side of a closing group (mu held): a block nobody is using -- never used, given back, or whose last launch is seen
// complete now (its owner then needs it no more) --, else a new one (its memory is allocated by the launch, outside the mutex)
Block *pick_block(symaccel_batcher *b, Group *g) {
    Block *found = nullptr;
    for (auto &up : b->blocks) {
        Block *k = up.get();
        if (k->owner == nullptr) {
            found = k;
            break;
        }
        Group *o = k->owner;
        if (o->state == GroupState::Launched && (o->completed || read_flag(k->h_flag) >= k->seq)) {  // (a read of host memory: no runtime call)
            o->completed = true;
            o->block = nullptr;
            found = k;
            break;
        }
    }
    if (!found) {
        void *h = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        std::memset(h, 0, 64);
        b->blocks.emplace_back(new Block());
        found = b->blocks.back().get();
        found->h_flag = static_cast<uint64_t *>(h);
        b->stats.blocks = b->blocks.size();
    }
    found->owner = g;
    found->seq += 1;
    g->block = found;
    g->completed = false;
    g->done_flag = found->h_flag;
    g->done_seq = found->seq;
    return found;
}

// the lane a closing group goes to (mu held): round robin over the lanes that exist; the second and later ones are made on demand
Lane *pick_lane(symaccel_batcher *b) {
    if (b->lanes.empty()) {
        b->lanes.emplace_back(new Lane());
        b->lanes.back()->ctx = b->ctx;
    }
    const size_t want = std::max<size_t>(1, b->want_lanes);
    const size_t idx = b->next_lane++ % want;
    while (b->lanes.size() <= idx) {
        symaccel_ctx *c = nullptr;
        if (symaccel_ctx_create(b->ctx->device, &c) != SYMACCEL_OK) {  // (no second context: everything stays on the lanes there are)
            b->want_lanes = b->lanes.size();
            return b->lanes[idx % b->lanes.size()].get();
        }
        c->segment = b->ctx->segment;
        b->lanes.emplace_back(new Lane());
        b->lanes.back()->ctx = c;
        b->lanes.back()->owned = true;
    }
    b->stats.lanes = b->lanes.size();
    return b->lanes[idx].get();
}

// mu held.  Close the group, wait until every reservation of it is filled, enqueue it on a lane WITHOUT the mutex.  On return the
// group is Launched (its status says whether the launch worked) -- or somebody else is launching / has launched it.
void flush_group(symaccel_batcher *b, Group *g, std::unique_lock<std::mutex> &lock) {
    if (g->state != GroupState::Open) return;
    if (g->tickets == 0) {  // (opened and never filled: nothing to launch, nobody to release it)
        g->state = GroupState::Free;
        return;
    }
    g->state = GroupState::Closed;
    b->cv.wait(lock, [&] { return g->uncommitted == 0; });
    if (g->state != GroupState::Closed) return;
    int st = SYMACCEL_OK;
    uint64_t chunks = 0, host_ns = 0, lane_ns = 0, api_ns = 0, allocs = 0;
    std::string err;
    if (g->tickets) {
        // what the launch needs of the batcher, copied while the mutex is still ours
        g->views.resize(g->tickets);
        const Clock::time_point closing = Clock::now();
        for (size_t i = 0; i < g->tickets; ++i) {
            const Ticket &t = b->tickets[g->ticket_ids[i]];
            g->views[i] = TicketView{t.slot, t.first_chain, t.n_chains, SYMACCEL_OK, t.out_fmt, t.channels};
            g->views[i].in_fmt = t.in_fmt;
            if (t.committed_at != Clock::time_point{}) b->stats.commit_to_launch_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(closing - t.committed_at).count();
        }
        if (g->kind == SYMACCEL_BATCH_AAC_DECODE && g->param >= 0) g->aac.maps = b->bands[(size_t)g->param].maps;  // (the index was checked by reserve())
        if (g->kind == SYMACCEL_BATCH_VORBIS_DECODE) g->vb.floors = b->floors;
        g->knobs = b->knobs;
        Lane *lane = pick_lane(b);
        g->lane = lane;
        if (!pick_block(b, g)) {  // (no page-locked word for a new block's completion flag)
            for (size_t i = 0; i < g->tickets; ++i) b->tickets[g->ticket_ids[i]].status = SYMACCEL_ERR_OOM;
            g->status = SYMACCEL_ERR_OOM;
            g->completed = true;
            g->state = GroupState::Launched;
            b->cv.notify_all();
            return;
        }
        g->state = GroupState::Launching;
        lock.unlock();
        {
            const Clock::time_point t0 = Clock::now();
            std::unique_lock<std::mutex> lane_lock(lane->mu);
            lane_ns = ns_since(t0);
            const Clock::time_point t1 = Clock::now();
            DeviceGuard dev(lane->ctx);
            st = dev.ok() ? launch_group_inner(lane, g, &chunks, &api_ns, &allocs) : dev.status();
            if (st != SYMACCEL_OK) {
                // a launch that failed half way: nothing of this group may still be in flight when its slots are reused, and the
                // copy-out stream does not follow what the other two were left with -- drain all three (error path only)
                err = lane->ctx->last_error;
                if (lane->ctx->stage_in) (void)hipStreamSynchronize(lane->ctx->stage_in);
                if (lane->ctx->stream) (void)hipStreamSynchronize(lane->ctx->stream);
                if (lane->ctx->stage_out) (void)hipStreamSynchronize(lane->ctx->stage_out);
            }
            // the completion flag is written behind the last scatter, which follows the last kernel, which follows the last gather
            if (st == SYMACCEL_OK) st = launch_batch_flag(lane->ctx, lane->ctx->stage_out, g->block->h_flag, g->done_seq);
            if (st != SYMACCEL_OK && err.empty()) {
                err = lane->ctx->last_error;
                if (lane->ctx->stage_out) (void)hipStreamSynchronize(lane->ctx->stage_out);
            }
            host_ns = ns_since(t1);
        }
        lock.lock();
        if (st != SYMACCEL_OK) {
            b->last_error = err;
            g->completed = true;  // (the lane's streams were drained)
        }
        for (size_t i = 0; i < g->tickets; ++i) {
            Ticket &t = b->tickets[g->ticket_ids[i]];
            t.status = st != SYMACCEL_OK ? st : g->views[i].status;
            if (t.out_fmt) t.out_valid = t.status == SYMACCEL_OK ? g->views[i].out_valid : 0;
            if (t.status != SYMACCEL_OK) b->stats.failed_tickets += 1;
        }
    }
    g->status = st;
    g->state = GroupState::Launched;
    g->launched_at = Clock::now();
    b->stats.launches += 1;
    b->stats.chunks += chunks;
    b->stats.launch_host_ns += host_ns;
    b->stats.launch_api_ns += api_ns;
    b->stats.group_allocs += allocs;
    b->stats.lane_wait_ns += lane_ns;
    b->stats.chains_launched += g->chains;
    b->stats.max_chains_per_launch = std::max<uint64_t>(b->stats.max_chains_per_launch, g->chains);
    b->cv.notify_all();
}

Group *open_group(symaccel_batcher *b, int kind, int param, size_t units, const PlaneSizes &ps, size_t n_chains) {
    Group *spare = nullptr;
    for (auto &up : b->groups) {
        Group *g = up.get();
        if (g->state == GroupState::Open && g->kind == kind && g->units == units) {
            if (g->param == param) return g;
            // AAC_DECODE: a submission without jointly coded pairs (param -1) reads no band table: it rides with whatever table the
            // group has, and a group that so far holds only such submissions takes the table of the first one that does need it
            if (kind == SYMACCEL_BATCH_AAC_DECODE && (param == -1 || g->param == -1)) {
                if (g->param == -1) g->param = param;
                return g;
            }
        }
        if (g->state == GroupState::Free && !spare) spare = g;
    }
    if (!spare) {
        b->groups.emplace_back(new Group());
        spare = b->groups.back().get();
    }
    Group *g = spare;
    g->kind = kind;
    g->units = units;
    g->ps = ps;
    g->param = param;
    // what a group takes before it is launched unasked: flush_bytes of input
    g->cap_chains = std::max<size_t>(n_chains, std::max<size_t>(2, flush_threshold(b->flush_bytes, kind) / std::max<size_t>(1, in_bytes_per_chain(ps))));
    g->chains = g->tickets = g->uncommitted = g->live = 0;
    g->ticket_ids.clear();
    g->status = SYMACCEL_OK;
    g->block = nullptr;
    g->completed = false;
    g->lane = nullptr;
    g->state = GroupState::Open;
    return g;
}

Ticket *find_ticket(symaccel_batcher *b, uint64_t id) {
    const uint32_t idx = (uint32_t)(id & 0xffffffffu), gen = (uint32_t)(id >> 32);
    if (idx >= b->tickets.size()) return nullptr;
    Ticket *t = &b->tickets[idx];
    return t->live && t->gen == gen ? t : nullptr;
}

void fill_slot(const Group *g, const Ticket *t, symaccel_batch_slot *slot) {
    const SlotLayout l = slot_layout(g->ps, t->n_chains);
    std::memset(slot, 0, sizeof(*slot));
    for (int i = 0; i < g->ps.n_in; ++i) {
        slot->input[i] = t->slot + l.in[i];
        slot->input_bytes[i] = l.in_bytes[i];
    }
    if (t->in_fmt == SYMACCEL_FMT_S16) slot->input_bytes[0] = l.in_bytes[0] / 2;  // (int16_t words: the front half of the native plane's region)
    if (t->in_fmt == SYMACCEL_IN_FMT_ROWS) {  // (rows at their native offsets: the region as it is; the width table behind the shape's planes)
        slot->input[5] = t->slot + l.bytes;
        slot->input_bytes[5] = t->n_chains;
    }
    for (int i = 0; i < g->ps.n_state; ++i) {
        slot->state[i] = t->slot + l.state[i];
        slot->state_bytes[i] = l.state_bytes[i];
    }
    slot->out = t->slot + l.out;
    slot->out_bytes = t->out_fmt ? t->out_valid : l.out_bytes;
}

// Wait until nothing of a launched group is in flight (no mutex held).  The launch's last kernel writes the group's sequence number
// into a word of page-locked memory: the waiter reads that word -- spinning briefly, then yielding, then sleeping in steps of 20 us
// -- and calls nothing in the runtime.  A word that never arrives (a hung or lost device) is a device error after `kFlagTimeout`.
constexpr double kFlagTimeout = 60.0;

int sync_done(symaccel_batcher *b, Group *g) {
    const uint64_t *flag;
    uint64_t seq;
    {
        Locked l(b);
        if (!g->tickets || g->completed || !g->done_flag) return SYMACCEL_OK;
        flag = g->done_flag;
        seq = g->done_seq;
    }
    const Clock::time_point t0 = Clock::now();
    for (unsigned spins = 0; read_flag(flag) < seq; ++spins) {
        if (spins < 2000) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        } else if (spins < 4000) {
            std::this_thread::yield();
        } else {
            std::this_thread::sleep_for(std::chrono::microseconds(20));
            if ((spins & 1023) == 0 && std::chrono::duration<double>(Clock::now() - t0).count() > kFlagTimeout) {
                Locked l(b);
                b->last_error = "the completion flag of a batch never arrived";
                return SYMACCEL_ERR_DEVICE;
            }
        }
    }
    Locked l(b);
    const uint64_t waited = ns_since(t0);
    b->stats.waits += 1;
    if (waited > 2000) {  // (the word was not there yet)
        b->stats.waits_blocked += 1;
        if (!g->completed) b->stats.launch_to_done_ns += ns_since(g->launched_at), b->stats.launches_timed += 1;  // (first to see it: enqueue -> completion seen)
    }
    g->completed = true;
    b->stats.flag_wait_ns += waited;
    return SYMACCEL_OK;
}

}  // namespace

extern "C" {

int symaccel_batcher_create(symaccel_ctx *ctx, size_t flush_bytes, symaccel_batcher **out) {
    if (!ctx || !out) return SYMACCEL_ERR_INVALID_ARG;
    *out = nullptr;
    symaccel_batcher *b = new (std::nothrow) symaccel_batcher();
    if (!b) return SYMACCEL_ERR_OOM;
    b->ctx = ctx;
    b->flush_bytes = flush_bytes ? flush_bytes : (size_t)64 << 20;
    b->hint_bytes = std::min<size_t>((size_t)4 << 20, b->flush_bytes / 8);
    if (const char *e = std::getenv("SYMACCEL_BATCHER_HINT_MB"))  // development knob (tools/gpu_r5g.sh): the hint threshold in MiB
        if (std::atoi(e) > 0) b->hint_bytes = (size_t)std::atoi(e) << 20;
    if (const char *e = std::getenv("SYMACCEL_BATCHER_BUSY_GROUPS"))  // development knobs: the busy rule of symaccel_batcher_hint (0 = off) ...
        b->busy_groups = (size_t)std::max(0, std::atoi(e));
    if (const char *e = std::getenv("SYMACCEL_BATCHER_BUSY_HINT_MB"))  // ... and its threshold
        if (std::atoi(e) > 0) b->busy_hint_bytes = (size_t)std::atoi(e) << 20;
    if (const char *e = std::getenv("SYMACCEL_BATCHER_LANES"))  // development knob: the number of lanes (symaccel_batcher_configure)
        if (std::atoi(e) > 0) b->want_lanes = std::min(8, std::atoi(e));
    if (const char *e = std::getenv("SYMACCEL_BATCH_ROW_PAD")) b->knobs.row_pad = std::atol(e) != 0;
    if (const char *e = std::getenv("SYMACCEL_BATCH_DMA_KB")) b->knobs.dma_bytes = (size_t)std::atol(e) << 10;
    if (const char *e = std::getenv("SYMACCEL_BATCH_CHUNKS")) b->knobs.chunk_div = (size_t)std::min(64L, std::max(1L, std::atol(e)));
    if (const char *e = std::getenv("SYMACCEL_BATCH_CHUNK_MIN_KB")) b->knobs.chunk_min = (size_t)std::max(64L, std::atol(e)) << 10;
    *out = b;
    return SYMACCEL_OK;
}

int symaccel_batcher_configure(symaccel_batcher *b, int lanes, size_t hint_bytes) {
    if (!b || lanes < 0 || lanes > 8) return SYMACCEL_ERR_INVALID_ARG;
    Locked l(b);
    if (lanes) b->want_lanes = (size_t)lanes;  // (lanes already made stay; fewer are used from now on)
    if (hint_bytes) b->hint_bytes = hint_bytes;
    return SYMACCEL_OK;
}

int symaccel_batcher_destroy(symaccel_batcher *b) {
    if (!b) return SYMACCEL_OK;
    {
        DeviceGuard dev(b->ctx);
        // nothing of ours may still be in flight when the staging memory goes
        for (auto &ln : b->lanes) {
            std::unique_lock<std::mutex> lane_lock(ln->mu);
            if (ln->ctx->stage_in) (void)hipStreamSynchronize(ln->ctx->stage_in);
            if (ln->ctx->stream) (void)hipStreamSynchronize(ln->ctx->stream);
            if (ln->ctx->stage_out) (void)hipStreamSynchronize(ln->ctx->stage_out);
        }
        for (auto &k : b->blocks) block_free(k.get());
        for (auto &sl : b->slabs) (void)hipHostFree(sl.base);
    }
    for (auto &ln : b->lanes)
        if (ln->owned) symaccel_ctx_destroy(ln->ctx);
    delete b;
    return SYMACCEL_OK;
}

int symaccel_batcher_reserve(symaccel_batcher *b, int kind, int param, size_t n_chains, size_t units_per_chain, symaccel_batch_slot *slot,
                             uint64_t *ticket) {
    return symaccel_batcher_reserve_fmt(b, kind, param, n_chains, units_per_chain, 0, 0, slot, ticket);
}

int symaccel_batcher_reserve_fmt(symaccel_batcher *b, int kind, int param, size_t n_chains, size_t units_per_chain, int out_fmt, int channels,
                                 symaccel_batch_slot *slot, uint64_t *ticket) {
    return symaccel_batcher_reserve_io(b, kind, param, n_chains, units_per_chain, 0, out_fmt, channels, slot, ticket);
}

int symaccel_batcher_reserve_io(symaccel_batcher *b, int kind, int param, size_t n_chains, size_t units_per_chain, int in_fmt, int out_fmt,
                                int channels, symaccel_batch_slot *slot, uint64_t *ticket) {
    // (the widening happens in the gather, before any kernel of the kind sees the plane: every param form of the two kinds takes it)
    if (in_fmt != 0 && ((in_fmt != SYMACCEL_FMT_S16 && in_fmt != SYMACCEL_IN_FMT_ROWS) || !serial_kind(kind))) return SYMACCEL_ERR_INVALID_ARG;
    if (!b || !slot || !ticket || n_chains == 0 || n_chains > 0x7fffffffu) return SYMACCEL_ERR_INVALID_ARG;
    // (a PCM packet of 0 frames is a packet like any other -- lib.rs:320: floor(len / frame bytes) -- with empty planes: it takes a ticket,
    // rides in the group of its shape and comes back with 0 bytes)
    if (units_per_chain == 0 && kind != SYMACCEL_BATCH_PCM_DECODE) return SYMACCEL_ERR_INVALID_ARG;
    if (kind == SYMACCEL_BATCH_ADPCM_DECODE) {
        // the interleave group is one block's channels, and the decode kernel itself writes the format: the format joins the group key,
        // and from here on the submission is an ordinary one whose output plane holds [chain][frame][channel] samples of out_fmt
        if (param < 0 || (param >> 16) || (out_fmt != 0 && (symaccel_sample_bytes(out_fmt) == 0 || channels != adpcm_param(param).nch))) return SYMACCEL_ERR_INVALID_ARG;
        param |= out_fmt << 16;
        out_fmt = channels = 0;
    }
    if (kind == SYMACCEL_BATCH_PCM_DECODE) {  // likewise: the interleave group is one packet's channels, the kernel writes the format
        if (param < 0 || (param >> 24) || (out_fmt != 0 && (symaccel_sample_bytes(out_fmt) == 0 || channels != pcmdec_param(param).nch))) return SYMACCEL_ERR_INVALID_ARG;
        param |= out_fmt << 24;
        out_fmt = channels = 0;
    }
    if (out_fmt != 0 && (symaccel_sample_bytes(out_fmt) == 0 || channels < 1 || channels > 8 || n_chains % (size_t)channels != 0)) return SYMACCEL_ERR_INVALID_ARG;
    PlaneSizes ps;
    if (kind == SYMACCEL_BATCH_AAC_SYNTH) param = 0;
    if (!plane_sizes(kind, param, units_per_chain, &ps)) return SYMACCEL_ERR_INVALID_ARG;
    if ((kind == SYMACCEL_BATCH_MP3_SYNTH || kind == SYMACCEL_BATCH_MP3_DECODE) && (param < 0 || param > 8)) return SYMACCEL_ERR_INVALID_ARG;  // sample_rate_idx
    if (kind == SYMACCEL_BATCH_MP3_DECODE && n_chains > 2) return SYMACCEL_ERR_INVALID_ARG;            // one stream per submission
    if (kind == SYMACCEL_BATCH_VORBIS_DECODE && n_chains != (size_t)vorbis_param(param, units_per_chain).nch) return SYMACCEL_ERR_INVALID_ARG;  // one stream per submission
    for (int i = 0; i < ps.n_in; ++i)
        if (n_chains % ps.in_div[i] != 0) return SYMACCEL_ERR_INVALID_ARG;  // channel pairs; whole frames of a verified FLAC stream
    if (kind == SYMACCEL_BATCH_FLAC_RESTORE && flac_verify_param(param).verify && out_fmt != 0) return SYMACCEL_ERR_INVALID_ARG;
    Locked locked(b);
    std::unique_lock<std::mutex> &lock = locked.lock;
    if (kind == SYMACCEL_BATCH_AAC_DECODE && param != -1 && (param < 0 || (size_t)param >= b->bands.size())) return SYMACCEL_ERR_INVALID_ARG;  // (symaccel_batcher_aac_bands first; -1: no pairs, no table)
    // the slot first: page-locking a new slab drops the mutex, and the group must be chosen in one piece with the reservation
    const SlotLayout lay = slot_layout(ps, n_chains);
    // (a ticket with a width per row: its width table behind the planes, slot.input[5] -- fill_slot, TicketView::row_bytes)
    const size_t cls = slot_class(lay.bytes + (in_fmt == SYMACCEL_IN_FMT_ROWS ? round256(n_chains) : 0));
    char *mem = nullptr;
    SYM_TRY(slot_alloc(b, lock, cls, &mem));
    Group *g = open_group(b, kind, param, units_per_chain, ps, n_chains);
    while (g->chains + n_chains > g->cap_chains && g->tickets) {  // full: it goes, a fresh one opens (or one somebody else opened meanwhile)
        flush_group(b, g, lock);
        g = open_group(b, kind, param, units_per_chain, ps, n_chains);
    }
    uint32_t idx;
    if (!b->free_tickets.empty()) {
        idx = b->free_tickets.back();
        b->free_tickets.pop_back();
    } else {
        idx = (uint32_t)b->tickets.size();
        b->tickets.emplace_back();
    }
    Ticket *t = &b->tickets[idx];
    const uint32_t gen = t->gen + 1;
    *t = Ticket();
    t->gen = gen;
    t->group = g;
    t->first_chain = (uint32_t)g->chains;
    t->n_chains = (uint32_t)n_chains;
    t->live = true;
    t->slot = mem;
    t->slot_bytes = cls;
    if (out_fmt) {  // (the native planes are 4 bytes a sample: the region reserved for them holds any format)
        t->out_fmt = out_fmt;
        t->channels = (uint32_t)channels;
        t->out_valid = lay.out_bytes / 4 * symaccel_sample_bytes(out_fmt);
    }
    t->in_fmt = in_fmt;
    g->ticket_ids.push_back(idx);
    g->chains += n_chains;
    g->tickets += 1;
    g->uncommitted += 1;
    g->live += 1;
    b->stats.submissions += 1;
    b->slots_live += 1;
    b->stats.slots_peak = std::max<uint64_t>(b->stats.slots_peak, b->slots_live);
    fill_slot(g, t, slot);
    *ticket = ((uint64_t)gen << 32) | idx;
    return SYMACCEL_OK;
}

int symaccel_batcher_commit(symaccel_batcher *b, uint64_t ticket) {
    if (!b) return SYMACCEL_ERR_INVALID_ARG;
    Locked locked(b);
    Ticket *t = find_ticket(b, ticket);
    if (!t || t->committed) return SYMACCEL_ERR_INVALID_ARG;
    t->committed = true;
    t->committed_at = Clock::now();
    Group *g = t->group;
    g->uncommitted -= 1;
    if (g->uncommitted == 0) b->cv.notify_all();
    // enough input has piled up: to the device, nobody has to ask
    if (g->state == GroupState::Open && g->chains * in_bytes_per_chain(g->ps) >= flush_threshold(b->flush_bytes, g->kind)) flush_group(b, g, locked.lock);
    return SYMACCEL_OK;
}

int symaccel_batcher_flush(symaccel_batcher *b) {
    if (!b) return SYMACCEL_ERR_INVALID_ARG;
    Locked locked(b);
    for (size_t i = 0; i < b->groups.size(); ++i)  // (index loop: flush_group drops the lock while it waits for commits and while it enqueues)
        if (b->groups[i]->state == GroupState::Open && b->groups[i]->tickets) flush_group(b, b->groups[i].get(), locked.lock);
    return SYMACCEL_OK;
}

int symaccel_batcher_hint(symaccel_batcher *b) {
    if (!b) return SYMACCEL_ERR_INVALID_ARG;
    Locked locked(b);
    // "results will be wanted soon": whatever is worth a launch of its own goes now, so that the copies and the kernels run while
    // the callers are still busy with their current batches; a group below that size waits for more submissions (or for a waiter).
    // What is worth a launch depends on the device: while it is idle a small group is (its latency is hidden behind the callers' work);
    // while it has a queue -- `busy_groups` launches whose completion word is outstanding (a read of page-locked memory) -- an early launch
    // buys nothing, and LARGER groups move faster: the copy kernels of a 6 MiB group carry 28 GB/s each way, those of a 40 MiB group 31
    // (AAC at S = 256: 3.45 -> 3.92 M packets/s, S = 64: 3.38 -> 3.62, S = 4: 1.78 -> 1.98; profiles/r06z1_hint.jsonl, r06z3_busy.jsonl)
    size_t in_flight = 0;
    for (auto &up : b->groups) {
        const Group *o = up.get();
        if (o->state == GroupState::Closed || o->state == GroupState::Launching) in_flight += 1;
        else if (o->state == GroupState::Launched && o->tickets && !o->completed && o->done_flag && read_flag(o->done_flag) < o->done_seq) in_flight += 1;
    }
    const bool busy = b->busy_groups && in_flight >= b->busy_groups;
    for (size_t i = 0; i < b->groups.size(); ++i) {
        Group *g = b->groups[i].get();
        size_t worth = hint_threshold(b->hint_bytes, b->flush_bytes, g->kind);
        if (busy) worth = std::max(worth, std::min(b->busy_hint_bytes, b->flush_bytes));
        if (g->state == GroupState::Open && g->tickets && g->chains * in_bytes_per_chain(g->ps) >= worth) flush_group(b, g, locked.lock);
    }
    return SYMACCEL_OK;
}

int symaccel_batcher_wait(symaccel_batcher *b, uint64_t ticket, symaccel_batch_slot *slot) {
    if (!b) return SYMACCEL_ERR_INVALID_ARG;
    Group *g;
    int status;
    {
        Locked locked(b);
        std::unique_lock<std::mutex> &lock = locked.lock;
        Ticket *t = find_ticket(b, ticket);
        if (!t || !t->committed) return SYMACCEL_ERR_INVALID_ARG;
        g = t->group;
        if (g->state == GroupState::Open) {
            // somebody needs a result: everything pending goes now -- the waiter's group first, then its siblings of other shapes,
            // which would otherwise each cost their first waiter a round trip of their own
            flush_group(b, g, lock);
            for (size_t i = 0; i < b->groups.size(); ++i)
                if (b->groups[i]->state == GroupState::Open && b->groups[i]->tickets) flush_group(b, b->groups[i].get(), lock);
        }
        b->cv.wait(lock, [&] { return g->state == GroupState::Launched; });
        t = find_ticket(b, ticket);  // (the table may have grown while the lock was dropped)
        if (!t) return SYMACCEL_ERR_INVALID_ARG;
        if (slot) fill_slot(g, t, slot);
        status = t->status;
    }
    const int st = sync_done(b, g);
    return st != SYMACCEL_OK ? st : status;
}

int symaccel_batcher_release(symaccel_batcher *b, uint64_t ticket) {
    if (!b) return SYMACCEL_ERR_INVALID_ARG;
    Locked locked(b);
    std::unique_lock<std::mutex> &lock = locked.lock;
    Ticket *t = find_ticket(b, ticket);
    if (!t) return SYMACCEL_ERR_INVALID_ARG;
    Group *g = t->group;
    if (!t->committed) {
        // abandoned before it was filled (a front end that threw half way): what the slot holds is whatever it is, and it will be
        // launched with its group -- as an EMPTY description: every plane zeroed (no pairs, no filters, verbatim blocks, silence), so
        // that the neighbours' launch never reads garbage descriptors.  Error path: the memset runs without the mutex (the group
        // cannot be launched while this reservation is open).
        char *mem = t->slot;
        const size_t bytes = slot_layout(g->ps, t->n_chains).bytes;
        lock.unlock();
        std::memset(mem, 0, bytes);
        lock.lock();
        t = find_ticket(b, ticket);
        if (!t) return SYMACCEL_ERR_INVALID_ARG;
        if (!t->committed) {
            t->committed = true;
            g->uncommitted -= 1;
            if (g->uncommitted == 0) b->cv.notify_all();
        }
    }
    // The slot goes back to the pool -- but the group's copies may still be reading or writing it (a release without a wait, or
    // before the launch): the group is launched if it has not been, and drained, first.  (The common order -- wait, read, release --
    // finds the event signalled.)
    if (g->state == GroupState::Open) flush_group(b, g, lock);
    b->cv.wait(lock, [&] { return g->state == GroupState::Launched; });
    if (g->tickets && !g->completed) {
        lock.unlock();
        (void)sync_done(b, g);
        lock.lock();
    }
    t = find_ticket(b, ticket);  // (the table may have grown while the lock was dropped)
    if (!t) return SYMACCEL_ERR_INVALID_ARG;
    slot_free(b, t->slot, t->slot_bytes);
    b->slots_live -= 1;
    t->slot = nullptr;
    t->live = false;
    b->free_tickets.push_back((uint32_t)(ticket & 0xffffffffu));
    g->live -= 1;
    if (g->live == 0 && g->state == GroupState::Launched) {
        // (every submission was drained before it was released: the launch is complete, its block serves the next one)
        if (g->block && g->block->owner == g) g->block->owner = nullptr;
        g->block = nullptr;
        g->state = GroupState::Free;
    }
    return SYMACCEL_OK;
}

int symaccel_batcher_plane_bytes(int kind, int param, size_t units_per_chain, size_t *in_bytes, size_t *state_bytes, size_t *out_bytes) {
    PlaneSizes ps;
    if (!plane_sizes(kind, param, units_per_chain, &ps)) return SYMACCEL_ERR_INVALID_ARG;
    for (int i = 0; i < kMaxIn; ++i)
        if (in_bytes) in_bytes[i] = ps.in[i];
    for (int i = 0; i < kMaxState; ++i)
        if (state_bytes) state_bytes[i] = ps.state[i];
    if (out_bytes) *out_bytes = ps.in_place ? ps.in[0] : ps.out;
    return SYMACCEL_OK;
}

int symaccel_batcher_submit(symaccel_batcher *b, int kind, int param, size_t n_chains, size_t units_per_chain, const void **in,
                            void **state_io, void *out, uint64_t *ticket) {
    return symaccel_batcher_submit_fmt(b, kind, param, n_chains, units_per_chain, in, state_io, out, 0, 0, ticket);
}

int symaccel_batcher_submit_fmt(symaccel_batcher *b, int kind, int param, size_t n_chains, size_t units_per_chain, const void **in,
                                void **state_io, void *out, int out_fmt, int channels, uint64_t *ticket) {
    return symaccel_batcher_submit_io(b, kind, param, n_chains, units_per_chain, in, state_io, out, 0, out_fmt, channels, ticket);
}

int symaccel_batcher_submit_io(symaccel_batcher *b, int kind, int param, size_t n_chains, size_t units_per_chain, const void **in,
                               void **state_io, void *out, int in_fmt, int out_fmt, int channels, uint64_t *ticket) {
    if (!b || !in || !state_io || !out || !ticket) return SYMACCEL_ERR_INVALID_ARG;
    if (kind == SYMACCEL_BATCH_AAC_DECODE) return SYMACCEL_ERR_INVALID_ARG;  // (symaccel_batcher_submit_aac_decode writes the blob)
    PlaneSizes ps;
    if (kind == SYMACCEL_BATCH_ADPCM_DECODE && (param < 0 || (param >> 16))) return SYMACCEL_ERR_INVALID_ARG;  // (the format travels in out_fmt)
    if (kind == SYMACCEL_BATCH_PCM_DECODE && (param < 0 || (param >> 24))) return SYMACCEL_ERR_INVALID_ARG;    // (likewise)
    if (!plane_sizes(kind, kind == SYMACCEL_BATCH_AAC_SYNTH ? 0 : param, units_per_chain, &ps)) return SYMACCEL_ERR_INVALID_ARG;
    for (int i = 0; i < ps.n_in; ++i)
        if (!in[i] && !(kind == SYMACCEL_BATCH_MP3_DECODE && i == 3 && n_chains == 1)) return SYMACCEL_ERR_INVALID_ARG;
    for (int i = 0; i < ps.n_state; ++i)
        if (!state_io[i]) return SYMACCEL_ERR_INVALID_ARG;
    const bool rows = in_fmt == SYMACCEL_IN_FMT_ROWS;
    if (rows && !in[5]) return SYMACCEL_ERR_INVALID_ARG;  // (the width table)
    symaccel_batch_slot slot;
    uint64_t id = 0;
    SYM_TRY(symaccel_batcher_reserve_io(b, kind, param, n_chains, units_per_chain, in_fmt, out_fmt, channels, &slot, &id));
    if (rows) {  // the width table, and of every row the bytes its width makes valid (none where the width is none of 2, 3, 4: the ticket fails)
        const uint8_t *w = static_cast<const uint8_t *>(in[5]);
        std::memcpy(slot.input[5], w, n_chains);
        for (size_t c = 0; c < n_chains; ++c)
            if (w[c] >= 2 && w[c] <= 4)
                std::memcpy(static_cast<char *>(slot.input[0]) + c * units_per_chain * 4, static_cast<const char *>(in[0]) + c * units_per_chain * 4, units_per_chain * w[c]);
    }
    for (int i = rows ? 1 : 0; i < ps.n_in; ++i) {
        if (in[i])
            std::memcpy(slot.input[i], in[i], slot.input_bytes[i]);
        else
            std::memset(slot.input[i], 0, slot.input_bytes[i]);
    }
    for (int i = 0; i < ps.n_state; ++i) std::memcpy(slot.state[i], state_io[i], slot.state_bytes[i]);
    {
        Locked locked(b);
        Ticket *t = find_ticket(b, id);
        for (int i = 0; i < ps.n_state; ++i) t->user_state[i] = state_io[i];
        t->user_out = out;
    }
    *ticket = id;
    return symaccel_batcher_commit(b, id);
}

int symaccel_batcher_submit_aac_synth(symaccel_batcher *b, const float *coeffs, const uint8_t *side, float *delay_io, float *pcm, size_t n_chains,
                                      size_t frames_per_chain, uint64_t *ticket) {
    const void *in[kMaxIn] = {coeffs, side, nullptr, nullptr, nullptr, nullptr};
    void *st[3] = {delay_io, nullptr, nullptr};
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_AAC_SYNTH, 0, n_chains, frames_per_chain, in, st, pcm, ticket);
}

int symaccel_batcher_submit_mp3_synth(symaccel_batcher *b, const float *xr, const symaccel_mp3_side *side, int sample_rate_idx, float *overlap_io,
                                      float *vvec_io, int32_t *vfront_io, float *pcm, size_t n_chains, size_t granules_per_chain, uint64_t *ticket) {
    const void *in[kMaxIn] = {xr, side, nullptr, nullptr, nullptr, nullptr};
    void *st[3] = {overlap_io, vvec_io, vfront_io};
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_MP3_SYNTH, sample_rate_idx, n_chains, granules_per_chain, in, st, pcm, ticket);
}

int symaccel_batcher_submit_mp3_decode(symaccel_batcher *b, const int16_t *quant, const symaccel_mp3_requant *rq_desc, const symaccel_mp3_stereo *st_desc,
                                       const symaccel_mp3_side *side, int sample_rate_idx, float *overlap_io, float *vvec_io, int32_t *vfront_io,
                                       float *pcm, size_t n_chains, size_t granules_per_chain, uint64_t *ticket) {
    const void *in[kMaxIn] = {quant, rq_desc, side, st_desc, nullptr, nullptr};
    void *st[3] = {overlap_io, vvec_io, vfront_io};
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_MP3_DECODE, sample_rate_idx, n_chains, granules_per_chain, in, st, pcm, ticket);
}

int symaccel_batcher_aac_bands(symaccel_batcher *b, const uint16_t *swb_long, int n_swb_long, const uint16_t *swb_short, int n_swb_short, int *bands) {
    if (!b || !bands || !swb_long || !swb_short || n_swb_long < 1 || n_swb_short < 1 || n_swb_long > 63 || n_swb_short > 15) return SYMACCEL_ERR_INVALID_ARG;
    symaccel_batcher::Bands nb;
    if (!aac_band_maps(swb_long, n_swb_long, swb_short, n_swb_short, &nb.maps)) return SYMACCEL_ERR_INVALID_ARG;
    nb.swb_long.assign(swb_long, swb_long + n_swb_long + 1);
    nb.swb_short.assign(swb_short, swb_short + n_swb_short + 1);
    Locked locked(b);
    for (size_t i = 0; i < b->bands.size(); ++i)
        if (b->bands[i].swb_long == nb.swb_long && b->bands[i].swb_short == nb.swb_short) {
            *bands = (int)i;
            return SYMACCEL_OK;
        }
    if (b->bands.size() >= 64) return SYMACCEL_ERR_UNSUPPORTED;
    b->bands.push_back(std::move(nb));
    *bands = (int)b->bands.size() - 1;
    return SYMACCEL_OK;
}

int symaccel_batcher_submit_aac_decode(symaccel_batcher *b, int bands, const float *coeffs, const uint8_t *side, const int32_t *pair_chains,
                                       const symaccel_aac_js_frame *js_desc, size_t n_pairs, const symaccel_aac_tns_filter *tns, size_t n_tns,
                                       float *delay_io, float *pcm, size_t n_chains, size_t frames_per_chain, uint64_t *ticket) {
    if (!b || !coeffs || !side || !delay_io || !pcm || !ticket || n_chains == 0 || frames_per_chain == 0) return SYMACCEL_ERR_INVALID_ARG;
    if ((n_pairs && (!pair_chains || !js_desc)) || (n_tns && !tns) || 2 * n_pairs > n_chains) return SYMACCEL_ERR_INVALID_ARG;
    {  // every chain in at most one pair, inside the submission (what symaccel_aac_decode_pipelined checks)
        std::vector<uint8_t> seen(n_chains, 0);
        for (size_t i = 0; i < 2 * n_pairs; ++i) {
            const int32_t c = pair_chains[i];
            if (c < 0 || (size_t)c >= n_chains || seen[(size_t)c]) return SYMACCEL_ERR_INVALID_ARG;
            seen[(size_t)c] = 1;
        }
    }
    PlaneSizes ps;
    if (!plane_sizes(SYMACCEL_BATCH_AAC_DECODE, bands, frames_per_chain, &ps)) return SYMACCEL_ERR_INVALID_ARG;
    if (aac_blob_bytes(n_pairs, frames_per_chain, n_tns) > ps.in[2] * n_chains) return SYMACCEL_ERR_INVALID_ARG;  // (more than 8 filters per channel-frame)
    symaccel_batch_slot slot;
    uint64_t id = 0;
    {
        Locked locked(b);
        if (bands != -1 && (bands < 0 || (size_t)bands >= b->bands.size())) return SYMACCEL_ERR_INVALID_ARG;  // (tables that were never registered)
    }
    // (a batch without a jointly coded pair reads no band table: it shares a launch with streams of any table)
    SYM_TRY(symaccel_batcher_reserve(b, SYMACCEL_BATCH_AAC_DECODE, n_pairs ? bands : -1, n_chains, frames_per_chain, &slot, &id));
    std::memcpy(slot.input[0], coeffs, slot.input_bytes[0]);
    std::memcpy(slot.input[1], side, slot.input_bytes[1]);
    char *blob = static_cast<char *>(slot.input[2]);
    AacBlobHeader h{(uint32_t)n_pairs, (uint32_t)n_tns, {0, 0}};
    std::memcpy(blob, &h, sizeof h);
    if (n_pairs) {
        std::memcpy(blob + aac_blob_pairs(n_pairs), pair_chains, n_pairs * 8);
        std::memcpy(blob + aac_blob_js(n_pairs), js_desc, n_pairs * frames_per_chain * sizeof(symaccel_aac_js_frame));
    }
    if (n_tns) std::memcpy(blob + aac_blob_tns(n_pairs, frames_per_chain), tns, n_tns * sizeof(symaccel_aac_tns_filter));
    std::memcpy(slot.state[0], delay_io, slot.state_bytes[0]);
    {
        Locked locked(b);
        Ticket *t = find_ticket(b, id);
        t->user_state[0] = delay_io;
        t->user_out = pcm;
    }
    *ticket = id;
    return symaccel_batcher_commit(b, id);
}

int symaccel_batcher_submit_vorbis_synth(symaccel_batcher *b, int bs0_exp, int bs1_exp, const float *spectra, const uint8_t *block_flag,
                                         int32_t *prev_flag_io, float *overlap_io, float *pcm, size_t n_chains, size_t blocks_per_chain,
                                         uint64_t *ticket) {
    if (bs0_exp < 0 || bs0_exp > 255 || bs1_exp < 0 || bs1_exp > 255) return SYMACCEL_ERR_INVALID_ARG;
    const void *in[kMaxIn] = {spectra, block_flag, nullptr, nullptr, nullptr, nullptr};
    void *st[3] = {prev_flag_io, overlap_io, nullptr};
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_VORBIS_SYNTH, bs0_exp | (bs1_exp << 8), n_chains, blocks_per_chain, in, st, pcm, ticket);
}

int symaccel_batcher_vorbis_floor(symaccel_batcher *b, const symaccel_vorbis_floor1_cfg *cfg, int *index) {
    if (!b || !cfg || !index) return SYMACCEL_ERR_INVALID_ARG;
    if (cfg->n_posts < 2 || cfg->n_posts > kVorbisPosts || cfg->multiplier < 1 || cfg->multiplier > 4) return SYMACCEL_ERR_INVALID_ARG;
    symaccel_vorbis_floor1_cfg c{};
    c.multiplier = cfg->multiplier;
    c.n_posts = cfg->n_posts;
    for (unsigned i = 0; i < cfg->n_posts; ++i) {
        if (cfg->x_list[i] > 0xffffu) return SYMACCEL_ERR_INVALID_ARG;  // floor1_X values have at most 15 bits (rangebits)
        for (unsigned j = 0; j < i; ++j)
            if (cfg->x_list[j] == cfg->x_list[i]) return SYMACCEL_ERR_INVALID_ARG;  // render_line divides by (x1 - x0)
        c.x_list[i] = cfg->x_list[i];
    }
    Locked locked(b);
    for (size_t i = 0; i < b->floors.size(); ++i)
        if (std::memcmp(&b->floors[i], &c, sizeof c) == 0) {
            *index = (int)i;
            return SYMACCEL_OK;
        }
    if (b->floors.size() >= SYMACCEL_VORBIS_FLOOR_UNUSED) return SYMACCEL_ERR_UNSUPPORTED;
    b->floors.push_back(c);
    *index = (int)b->floors.size() - 1;
    return SYMACCEL_OK;
}

int symaccel_batcher_submit_vorbis_decode(symaccel_batcher *b, int bs0_exp, int bs1_exp, const float *residue, const uint8_t *block_flag,
                                          const uint8_t *floor, const uint32_t *posts, const uint8_t *coupling, const uint32_t *coupling_first,
                                          int32_t *prev_flag_io, float *overlap_io, float *pcm, size_t n_chains, size_t blocks_per_chain,
                                          uint64_t *ticket) {
    if (!b || !residue || !block_flag || !floor || !posts || !coupling_first || !prev_flag_io || !overlap_io || !pcm || !ticket) return SYMACCEL_ERR_INVALID_ARG;
    if (bs0_exp < 0 || bs0_exp > 255 || bs1_exp < 0 || bs1_exp > 255 || n_chains == 0 || n_chains > 255 || blocks_per_chain == 0) return SYMACCEL_ERR_INVALID_ARG;
    const int param = bs0_exp | (bs1_exp << 8) | ((int)n_chains << 16);
    PlaneSizes ps;
    if (!plane_sizes(SYMACCEL_BATCH_VORBIS_DECODE, param, blocks_per_chain, &ps)) return SYMACCEL_ERR_INVALID_ARG;
    const size_t n_steps = coupling_first[blocks_per_chain];
    if ((n_steps && !coupling) || vorbis_blob_steps(blocks_per_chain) + 2 * n_steps > ps.in[4]) return SYMACCEL_ERR_INVALID_ARG;
    symaccel_batch_slot slot;
    uint64_t id = 0;
    SYM_TRY(symaccel_batcher_reserve(b, SYMACCEL_BATCH_VORBIS_DECODE, param, n_chains, blocks_per_chain, &slot, &id));
    std::memcpy(slot.input[0], residue, slot.input_bytes[0]);
    std::memcpy(slot.input[1], block_flag, slot.input_bytes[1]);
    std::memcpy(slot.input[2], floor, slot.input_bytes[2]);
    std::memcpy(slot.input[3], posts, slot.input_bytes[3]);
    char *blob = static_cast<char *>(slot.input[4]);
    std::memcpy(blob, coupling_first, (blocks_per_chain + 1) * 4);
    if (n_steps) std::memcpy(blob + vorbis_blob_steps(blocks_per_chain), coupling, 2 * n_steps);
    std::memcpy(slot.state[0], prev_flag_io, slot.state_bytes[0]);
    std::memcpy(slot.state[1], overlap_io, slot.state_bytes[1]);
    {
        Locked locked(b);
        Ticket *t = find_ticket(b, id);
        t->user_state[0] = prev_flag_io;
        t->user_state[1] = overlap_io;
        t->user_out = pcm;
    }
    *ticket = id;
    return symaccel_batcher_commit(b, id);
}

int symaccel_batcher_submit_flac_restore(symaccel_batcher *b, int32_t *buf_io, const symaccel_flac_desc *desc, const int32_t *coeffs,
                                         const uint8_t *pair_mode, uint32_t out_shift, size_t n_blocks, size_t blocksize, uint64_t *ticket) {
    if (out_shift > 31 || (!pair_mode && out_shift)) return SYMACCEL_ERR_INVALID_ARG;
    const void *in[kMaxIn] = {buf_io, desc, coeffs, pair_mode, nullptr, nullptr};
    void *st[3] = {nullptr, nullptr, nullptr};
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_FLAC_RESTORE, pair_mode ? (int)(0x100 | out_shift) : 0, n_blocks, blocksize, in, st, buf_io, ticket);
}

int symaccel_batcher_submit_flac_verify(symaccel_batcher *b, int32_t *buf_io, const symaccel_flac_desc *desc, const int32_t *coeffs,
                                        const symaccel_flac_md5_frame *frames, size_t n_frames, int nch, size_t blocksize, int finish, uint32_t out_shift,
                                        symaccel_md5_state *md5_states_io, uint64_t *ticket) {
    if (nch < 1 || nch > 8 || out_shift > 31 || (!finish && out_shift) || n_frames > 0x7fffffffu / 8) return SYMACCEL_ERR_INVALID_ARG;
    const void *in[kMaxIn] = {buf_io, desc, coeffs, frames, nullptr, nullptr};
    void *st[3] = {md5_states_io, nullptr, nullptr};
    const int param = (finish ? (int)(0x300 | out_shift) : 0x200) | (nch - 1) << 12;
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_FLAC_RESTORE, param, n_frames * (size_t)nch, blocksize, in, st, buf_io, ticket);
}

int symaccel_batcher_submit_adpcm_decode(symaccel_batcher *b, const uint8_t *bytes, int codec, size_t channels, size_t n_blocks, size_t block_bytes,
                                        int32_t *pcm, uint64_t *ticket) {
    if (codec < 0 || codec > 255 || channels > 255) return SYMACCEL_ERR_INVALID_ARG;
    const void *in[kMaxIn] = {bytes, nullptr, nullptr, nullptr, nullptr, nullptr};
    void *st[3] = {nullptr, nullptr, nullptr};
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_ADPCM_DECODE, codec | (int)(channels << 8), n_blocks, block_bytes, in, st, pcm, ticket);
}

int symaccel_batcher_submit_pcm_decode(symaccel_batcher *b, const uint8_t *bytes, int codec, size_t channels, uint32_t shift, size_t n_packets,
                                       size_t frames, void *pcm, uint64_t *ticket) {
    if (codec < 0 || codec > 255 || channels > 255 || shift > 255) return SYMACCEL_ERR_INVALID_ARG;
    const void *in[kMaxIn] = {bytes, nullptr, nullptr, nullptr, nullptr, nullptr};
    void *st[3] = {nullptr, nullptr, nullptr};
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_PCM_DECODE, codec | (int)(channels << 8) | (int)(shift << 16), n_packets, frames, in, st, pcm, ticket);
}

int symaccel_batcher_submit_alac_predict(symaccel_batcher *b, int32_t *buf_io, const symaccel_alac_desc *desc, const int32_t *coeffs,
                                         const int32_t *pair_weight, const uint8_t *pair_shift, size_t n_blocks, size_t blocksize, uint64_t *ticket) {
    if ((pair_weight == nullptr) != (pair_shift == nullptr)) return SYMACCEL_ERR_INVALID_ARG;
    const void *in[kMaxIn] = {buf_io, desc, coeffs, pair_weight, pair_shift, nullptr};
    void *st[3] = {nullptr, nullptr, nullptr};
    return symaccel_batcher_submit(b, SYMACCEL_BATCH_ALAC_PREDICT, pair_weight ? 0x100 : 0, n_blocks, blocksize, in, st, buf_io, ticket);
}

int symaccel_host_narrow_s16(const int32_t *src, int16_t *dst, size_t n) {
    if (n && (!src || !dst)) return 0;
    // one pass: every word is written as it is read, and what did not fit is OR-ed up -- no branch in the loop, so it vectorises
    uint32_t miss = 0;
    for (size_t i = 0; i < n; ++i) {
        const int32_t v = src[i];
        dst[i] = (int16_t)v;
        miss |= (uint32_t)v ^ (uint32_t)(int32_t)(int16_t)v;
    }
    return miss == 0;
}

int symaccel_host_pack_row(const int32_t *src, void *dst, size_t n) {
    if (n && (!src || !dst)) return 0;
    // the width first: v ^ (v >> 31) is v for v >= 0 and -v - 1 below, so the OR of all of them is below 2^15 (2^23) exactly when every
    // word fits 16 (24) bits -- no branch in the loop, so it vectorises; then the row at that width
    uint32_t mag = 0;
    for (size_t i = 0; i < n; ++i) mag |= (uint32_t)(src[i] ^ (src[i] >> 31));
    if (mag < 0x8000u) {
        int16_t *d = static_cast<int16_t *>(dst);
        for (size_t i = 0; i < n; ++i) d[i] = (int16_t)src[i];
        return 2;
    }
    if (mag < 0x800000u) {
        uint8_t *d = static_cast<uint8_t *>(dst);
        size_t i = 0;
        for (; i + 4 <= n; i += 4) {  // four words, three dwords: a quarter of the stores of the byte-by-byte form
            const uint32_t a = (uint32_t)src[i], b = (uint32_t)src[i + 1], c = (uint32_t)src[i + 2], e = (uint32_t)src[i + 3];
            const uint32_t q[3] = {(a & 0xffffffu) | (b << 24), ((b >> 8) & 0xffffu) | (c << 16), ((c >> 16) & 0xffu) | (e << 8)};
            std::memcpy(d + 3 * i, q, 12);
        }
        for (; i < n; ++i) {
            const uint32_t v = (uint32_t)src[i];
            d[3 * i] = (uint8_t)v, d[3 * i + 1] = (uint8_t)(v >> 8), d[3 * i + 2] = (uint8_t)(v >> 16);
        }
        return 3;
    }
    std::memcpy(dst, src, n * 4);
    return 4;
}

int symaccel_batcher_collect(symaccel_batcher *b, uint64_t ticket) {
    if (!b) return SYMACCEL_ERR_INVALID_ARG;
    symaccel_batch_slot slot;
    void *user_state[kMaxState], *user_out;
    bool verify;
    {
        Locked locked(b);
        Ticket *t = find_ticket(b, ticket);
        if (!t || !t->user_out) return SYMACCEL_ERR_INVALID_ARG;
        verify = t->group->kind == SYMACCEL_BATCH_FLAC_RESTORE && flac_verify_param(t->group->param).verify;
        for (int i = 0; i < kMaxState; ++i) user_state[i] = t->user_state[i];
        user_out = t->user_out;
    }
    const int st = symaccel_batcher_wait(b, ticket, &slot);
    if (st == SYMACCEL_OK) {
        std::memcpy(user_out, slot.out, slot.out_bytes);
        for (int i = 0; i < kMaxState; ++i)
            if (user_state[i] && slot.state[i]) std::memcpy(user_state[i], slot.state[i], slot.state_bytes[i]);
    } else if (verify && st == SYMACCEL_ERR_INVALID_ARG && user_state[0] && slot.state[0]) {
        std::memcpy(user_state[0], slot.state[0], slot.state_bytes[0]);  // (failed alone: every entry is the starting state)
    }
    const int rel = symaccel_batcher_release(b, ticket);
    return st != SYMACCEL_OK ? st : rel;
}

int symaccel_batcher_abandon(symaccel_batcher *b, uint64_t ticket) {
    if (!b) return SYMACCEL_ERR_INVALID_ARG;
    return symaccel_batcher_release(b, ticket);  // (release drains the ticket's group before the slot goes back)
}

int symaccel_batcher_get_stats(symaccel_batcher *b, symaccel_batcher_stats *out) {
    if (!b || !out) return SYMACCEL_ERR_INVALID_ARG;
    Locked locked(b);
    *out = b->stats;
    uint64_t pending = 0;
    for (auto &g : b->groups)
        if (g->state == GroupState::Open || g->state == GroupState::Closed) pending += g->tickets;
    out->pending = pending;
    return SYMACCEL_OK;
}

int symaccel_batcher_last_error(symaccel_batcher *b, char *buf, size_t capacity) {
    if (!b || !buf || capacity == 0) return SYMACCEL_ERR_INVALID_ARG;
    Locked locked(b);
    const size_t n = std::min(capacity - 1, b->last_error.size());
    std::memcpy(buf, b->last_error.data(), n);
    buf[n] = 0;
    return SYMACCEL_OK;
}

}  // extern "C"
