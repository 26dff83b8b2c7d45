//! Safe ownership of a `symaccel_ctx` and of page-locked batch buffers: `Context`, the process-wide `Pool`, a `BatchSlot` of the
//! cross-stream batcher and the `SlotCycle` through which the seven slot codecs hold theirs (AAC uses the copying ticket path), `Pinned`.
use std::ffi::CStr;
use std::ptr;
use std::sync::{Arc, Mutex};

use symphonia_core::errors::{unsupported_error, Error, Result};

use crate::ffi;

/// Map a symaccel status to the reference's error convention (include/symaccel.h, "Conventions";
/// symphonia-core/src/errors.rs:38-54): INVALID_ARG is the assert!/panic class, UNSUPPORTED -> Error::Unsupported,
/// DECODE -> Error::DecodeError (discard the packet, keep going), DEVICE / OOM -> Error::IoError.
pub(crate) fn check(status: i32, ctx: *const ffi::SymaccelCtx) -> Result<()> {
    if status >= 0 {
        return Ok(());
    }
    // SAFETY: symaccel_strerror returns a pointer to a static NUL-terminated string.
    let msg: &'static str = unsafe { CStr::from_ptr(ffi::symaccel_strerror(status)) }.to_str().unwrap_or("symaccel: error");
    match status {
        ffi::SYMACCEL_ERR_INVALID_ARG => panic!("{msg}"),
        ffi::SYMACCEL_ERR_UNSUPPORTED => Err(Error::Unsupported(msg)),
        ffi::SYMACCEL_ERR_DECODE => Err(Error::DecodeError(msg)),
        _ => {
            let detail = if ctx.is_null() {
                String::new()
            }
            else {
                // SAFETY: the context outlives this call; the string lives inside it.
                let text = unsafe { CStr::from_ptr(ffi::symaccel_last_error(ctx)) };
                text.to_string_lossy().into_owned()
            };
            Err(Error::IoError(std::io::Error::other(format!("{msg}: {detail}"))))
        }
    }
}

/// One HIP device + stream + constant tables.  `&mut self` on the decoders gives the external synchronisation the C
/// ABI asks for; the raw pointer is `Send + Sync` because the library is thread-safe across contexts and a context is
/// only ever touched through `&mut`.
pub struct Context {
    raw: *mut ffi::SymaccelCtx,
}

unsafe impl Send for Context {}
unsafe impl Sync for Context {}

impl Context {
    pub fn new(device: i32) -> Result<Self> {
        let mut raw = ptr::null_mut();
        // SAFETY: `raw` is a valid out-pointer.
        check(unsafe { ffi::symaccel_ctx_create(device, &mut raw) }, ptr::null())?;
        Ok(Context { raw })
    }

    pub(crate) fn raw(&self) -> *mut ffi::SymaccelCtx {
        self.raw
    }
}

impl Drop for Context {
    fn drop(&mut self) {
        // SAFETY: created by symaccel_ctx_create, destroyed once.
        unsafe { ffi::symaccel_ctx_destroy(self.raw) }
    }
}

/// The process-wide cross-stream batcher (csrc/batcher.cpp): ONE context and one `symaccel_batcher` shared by every pooled
/// decoder of the process.  A decoder cannot see its siblings (codecs/audio.rs:279-297, registry.rs:330-341); the pool is where
/// their look-ahead batches meet and go to the device in one launch.  The batcher is thread-safe; the pool's context is driven
/// through the batcher only.
pub struct Pool {
    batcher: *mut ffi::SymaccelBatcher,
    ctx: Context, // (declared after `batcher`: Drop destroys the batcher first, then the field drops the context)
    /// SYMACCEL_NARROW_INPUT, read once when the pool is made: how the FLAC / ALAC decoders send their words up.  Unset or 0: wide, every
    /// batch as `i32`.  2: a width per row (`SYMACCEL_IN_FMT_ROWS`), every subframe at the narrowest of 2, 3 or 4 bytes a word that holds
    /// it.  Anything else (1): a batch whose every word fits `i16` goes up as `i16`, any other wide (`symaccel_batcher_reserve_io`).
    input_mode: u8,
}

unsafe impl Send for Pool {}
unsafe impl Sync for Pool {}

static POOL: Mutex<Option<Arc<Pool>>> = Mutex::new(None);
static POOL_DEVICE: Mutex<i32> = Mutex::new(0);

impl Pool {
    /// The device the shared pool is created on (default 0).  One process per GPU: a launcher that does not narrow the visible
    /// devices per rank calls this with the local rank BEFORE `register()` / the first decoder; once the pool exists it stays
    /// where it is and the call returns `false`.
    pub fn set_device(device: i32) -> bool {
        let slot = POOL.lock().expect("pool poisoned");
        if slot.is_some() {
            return false;
        }
        *POOL_DEVICE.lock().expect("pool poisoned") = device;
        true
    }

    /// The shared pool, created on first use (the device of `set_device`, the library's default flush size).
    pub fn shared() -> Result<Arc<Pool>> {
        let mut slot = POOL.lock().expect("pool poisoned");
        if let Some(pool) = slot.as_ref() {
            return Ok(pool.clone());
        }
        let device = *POOL_DEVICE.lock().expect("pool poisoned");
        let ctx = Context::new(device)?;
        let mut batcher = ptr::null_mut();
        // SAFETY: valid context, valid out-pointer.
        check(unsafe { ffi::symaccel_batcher_create(ctx.raw(), 0, &mut batcher) }, ctx.raw())?;
        let input_mode: u8 = match std::env::var("SYMACCEL_NARROW_INPUT") {
            Ok(v) => {
                if v == "2" {
                    2
                } else if !v.is_empty() && v != "0" {
                    1
                } else {
                    0
                }
            }
            Err(_) => 0,
        };
        let pool = Arc::new(Pool { batcher, ctx, input_mode });
        *slot = Some(pool.clone());
        Ok(pool)
    }

    /// Do the FLAC / ALAC decoders of this pool narrow whole batches (SYMACCEL_NARROW_INPUT=1 at its creation)?
    pub fn narrow_input(&self) -> bool {
        self.input_mode == 1
    }

    /// SYMACCEL_NARROW_INPUT at the pool's creation: 0 = wide, 1 = whole batches as `i16` when they fit, 2 = a width per row.
    pub fn input_mode(&self) -> u8 {
        self.input_mode
    }

    pub(crate) fn raw(&self) -> *mut ffi::SymaccelBatcher {
        self.batcher
    }

    pub(crate) fn ctx_raw(&self) -> *mut ffi::SymaccelCtx {
        self.ctx.raw()
    }
}

/// A reservation with the cross-stream batcher (`symaccel_batcher_reserve`): a slot of page-locked staging memory the front end's
/// output is written STRAIGHT into -- the planes of the entry point the batch kind stands for, chain-major over this submission's
/// chains (include/symaccel.h, "cross-stream batcher") -- and the ticket that names it.  `Pool::commit` says it is filled,
/// `Pool::wait` blocks until `out` / `state` hold the PCM and the state after the batch (whatever the decoders of the OTHER streams
/// had pending went to the device in the same launch), `Pool::release` gives the slot back.  Nothing is copied between the parser's
/// output and the DMA source, and nothing between the DMA target and `AudioBuffer`'s planes but `publish`'s own plane copies.
pub struct BatchSlot {
    raw: ffi::SymaccelBatchSlot,
    ticket: u64,
    committed: bool,
}

// SAFETY: the slot's planes are owned by this reservation until `Pool::release`; the batcher itself is thread-safe.
unsafe impl Send for BatchSlot {}
unsafe impl Sync for BatchSlot {}

impl BatchSlot {
    /// Plane `i` of the submission's input as elements of `T` (the kind's layout: f32 spectra, u8 flags, #[repr(C)] records ...).
    pub fn input<T: Copy>(&mut self, i: usize) -> &mut [T] {
        // SAFETY: the batcher handed out `input_bytes[i]` bytes at `input[i]`, 256-byte aligned, exclusively ours until release.
        unsafe { std::slice::from_raw_parts_mut(self.raw.input[i] as *mut T, self.raw.input_bytes[i] / std::mem::size_of::<T>()) }
    }

    /// State plane `i`: the state the batch starts from (written before `commit`), the state it left (after `wait`).
    pub fn state<T: Copy>(&mut self, i: usize) -> &mut [T] {
        // SAFETY: as `input`.
        unsafe { std::slice::from_raw_parts_mut(self.raw.state[i] as *mut T, self.raw.state_bytes[i] / std::mem::size_of::<T>()) }
    }

    /// The result plane (after `wait`).  FLAC / ALAC work in place: it is input plane 0.
    pub fn out<T: Copy>(&self) -> &[T] {
        // SAFETY: as `input`; written by the device before `wait` returned.
        unsafe { std::slice::from_raw_parts(self.raw.out as *const T, self.raw.out_bytes / std::mem::size_of::<T>()) }
    }

    /// The result plane for a codec that finishes a packet in place in it (ALAC).  Not `input(0)`: a slot whose plane 0 went up as
    /// `i16` (`Pool::reserve_io`) has half as many input bytes as result bytes.
    pub fn out_mut<T: Copy>(&mut self) -> &mut [T] {
        // SAFETY: as `out`; exclusively ours until release.
        unsafe { std::slice::from_raw_parts_mut(self.raw.out as *mut T, self.raw.out_bytes / std::mem::size_of::<T>()) }
    }

    pub fn is_committed(&self) -> bool {
        self.committed
    }
}

impl Pool {
    /// `check` for calls into the batcher: a device error's text is the BATCHER's (`symaccel_batcher_last_error`, copied under its
    /// mutex) -- the shared context's own error string may be written by another thread's launch at any time.
    fn check(&self, status: i32) -> Result<()> {
        if status >= 0 || status == ffi::SYMACCEL_ERR_INVALID_ARG || status == ffi::SYMACCEL_ERR_UNSUPPORTED || status == ffi::SYMACCEL_ERR_DECODE {
            return check(status, ptr::null());
        }
        let mut text = [0 as core::ffi::c_char; 256];
        // SAFETY: a live batcher; `text` has room for 256 bytes including the terminator the library writes.
        unsafe { ffi::symaccel_batcher_last_error(self.batcher, text.as_mut_ptr(), text.len()) };
        // SAFETY: NUL-terminated by the library (or all zeros).
        let detail = unsafe { CStr::from_ptr(text.as_ptr()) }.to_string_lossy().into_owned();
        // SAFETY: symaccel_strerror returns a pointer to a static NUL-terminated string.
        let msg = unsafe { CStr::from_ptr(ffi::symaccel_strerror(status)) }.to_str().unwrap_or("symaccel: error");
        Err(Error::IoError(std::io::Error::other(format!("{msg}: {detail}"))))
    }

    /// `symaccel_batcher_reserve`: a slot for `n_chains` chains of `units` frames / granules / blocks / words each.
    pub fn reserve(&self, kind: i32, param: i32, n_chains: usize, units: usize) -> Result<BatchSlot> {
        self.reserve_io(kind, param, n_chains, units, 0)
    }

    /// `symaccel_batcher_reserve_io`: `in_fmt` `SYMACCEL_FMT_S16` (FLAC_RESTORE / ALAC_PREDICT) makes input plane 0 a plane of `i16`
    /// words, widened by the gather of the launch; 0 is `reserve`.
    pub fn reserve_io(&self, kind: i32, param: i32, n_chains: usize, units: usize, in_fmt: i32) -> Result<BatchSlot> {
        let mut raw = ffi::SymaccelBatchSlot {
            input: [ptr::null_mut(); 6],
            state: [ptr::null_mut(); 3],
            out: ptr::null_mut(),
            input_bytes: [0; 6],
            state_bytes: [0; 3],
            out_bytes: 0,
        };
        let mut ticket = 0u64;
        // SAFETY: a live batcher, valid out-pointers.
        self.check(unsafe {
            if in_fmt == 0 {
                ffi::symaccel_batcher_reserve(self.batcher, kind, param, n_chains, units, &mut raw, &mut ticket)
            } else {
                ffi::symaccel_batcher_reserve_io(self.batcher, kind, param, n_chains, units, in_fmt, 0, 0, &mut raw, &mut ticket)
            }
        })?;
        Ok(BatchSlot { raw, ticket, committed: false })
    }

    /// The slot is filled: it goes to the device with the next launch of its group.
    pub fn commit(&self, slot: &mut BatchSlot) -> Result<()> {
        // SAFETY: a live ticket of this batcher.
        self.check(unsafe { ffi::symaccel_batcher_commit(self.batcher, slot.ticket) })?;
        slot.committed = true;
        Ok(())
    }

    /// Block until the submission's results are in its slot.  The status is this submission's own: a batch whose descriptors do
    /// not add up fails alone, the neighbours of its launch do not (include/symaccel.h, "Status is kept PER TICKET").
    pub fn wait(&self, slot: &mut BatchSlot) -> Result<()> {
        let status = self.wait_raw(slot);
        self.check(status)
    }

    /// `wait` before the status is judged (`check` panics on INVALID_ARG: a caller that owns the slot gives it back first).
    fn wait_raw(&self, slot: &mut BatchSlot) -> i32 {
        // SAFETY: a live, committed ticket; the slot record is filled in again with the same pointers.
        unsafe { ffi::symaccel_batcher_wait(self.batcher, slot.ticket, &mut slot.raw) }
    }

    /// Give the slot back (a reservation that was never committed runs as zeros with its group; nobody looks at the result).
    pub fn release(&self, slot: BatchSlot) {
        // SAFETY: a live ticket; the batcher drains whatever of it is in flight before the memory is reused.
        unsafe { ffi::symaccel_batcher_release(self.batcher, slot.ticket) };
    }

    /// "Results will be wanted soon": pending groups worth a launch of their own go to the device now.
    pub fn hint(&self) {
        // SAFETY: a live batcher.
        unsafe { ffi::symaccel_batcher_hint(self.batcher) };
    }

    /// `symaccel_batcher_get_stats`: submissions, launches, what the callers waited for (mutex, lanes, completion flags).
    pub fn stats(&self) -> Result<ffi::SymaccelBatcherStats> {
        let mut s = ffi::SymaccelBatcherStats {
            submissions: 0,
            launches: 0,
            chunks: 0,
            chains_launched: 0,
            max_chains_per_launch: 0,
            staging_bytes: 0,
            pending: 0,
            failed_tickets: 0,
            lanes: 0,
            mutex_wait_ns: 0,
            mutex_contended: 0,
            launch_host_ns: 0,
            lane_wait_ns: 0,
            launch_api_ns: 0,
            group_allocs: 0,
            flag_wait_ns: 0,
            slots_peak: 0,
            blocks: 0,
            commit_to_launch_ns: 0,
            waits: 0,
            waits_blocked: 0,
            launch_to_done_ns: 0,
            launches_timed: 0,
        };
        // SAFETY: a live batcher, a valid out-pointer.
        self.check(unsafe { ffi::symaccel_batcher_get_stats(self.batcher, &mut s) })?;
        Ok(s)
    }

    /// Register a floor-1 configuration of a Vorbis stream's setup header; the index goes into the `floor` plane of the stream's
    /// `SYMACCEL_BATCH_VORBIS_DECODE` submissions.  The same configuration gives the same index in every stream.
    pub fn vorbis_floor(&self, cfg: &ffi::SymaccelVorbisFloor1Cfg) -> Result<u8> {
        let mut index: i32 = -1;
        // SAFETY: a live batcher, a valid record, a valid out-pointer.
        self.check(unsafe { ffi::symaccel_batcher_vorbis_floor(self.batcher, cfg, &mut index) })?;
        Ok(index as u8)
    }
}

impl Drop for Pool {
    fn drop(&mut self) {
        // SAFETY: created by symaccel_batcher_create, destroyed once, before its context.
        unsafe { ffi::symaccel_batcher_destroy(self.batcher) };
    }
}

/// The batcher-slot cycle of a pooled codec: the one place where `BatchSlot`s are reserved, committed, waited for and released.
///
/// A pooled codec has at most two slots at a time: the one whose batch is being handed out (`publish` reads the PCM where the device
/// left it) and the one submitted ahead.  The slots are page-locked memory that every stream of the process shares, so the rule is:
/// every slot is released exactly once, on every path.  `SlotCycle` owns the pool handle and both slots and is the only caller of
/// `Pool::reserve` / `commit` / `wait` / `release`; a codec supplies what is its own -- the kind, the parameter, the sizes, the fill of
/// the input planes, the read-back of the state planes -- and the per-batch index `M` (block sizes, trims, offsets: whatever its
/// `publish` needs to find a packet in the batch), which travels WITH the slot of its batch and becomes current when that slot does.
pub struct SlotCycle<M> {
    pool: Option<Arc<Pool>>,
    /// the index of the batch being handed out, and the slot it came in (`None`: a direct batch, served from the codec's own buffers)
    index: M,
    cur: Option<BatchSlot>,
    /// the batch submitted ahead and its index
    next: Option<(BatchSlot, M)>,
}

impl<M> SlotCycle<M> {
    /// `index`: what `index()` answers before the first batch (an empty one).
    pub fn new(pool: Option<Arc<Pool>>, index: M) -> Self {
        SlotCycle { pool, index, cur: None, next: None }
    }

    /// Does the codec submit to the shared batcher?
    pub fn pooled(&self) -> bool {
        self.pool.is_some()
    }

    /// The index of the batch being handed out.
    pub fn index(&self) -> &M {
        &self.index
    }

    /// The result plane of the batch being handed out, if it came through the batcher (read in place: nothing is copied).
    pub fn out<T: Copy>(&self) -> Option<&[T]> {
        match &self.cur {
            Some(slot) => Some(slot.out::<T>()),
            None => None,
        }
    }

    /// The current index together with the current slot, for a codec that finishes a packet in place in the slot (ALAC).
    pub fn parts_mut(&mut self) -> (&M, Option<&mut BatchSlot>) {
        (&self.index, self.cur.as_mut())
    }

    /// A batch the codec transforms on its own becomes current: a slot left from the batcher is done with and goes back.
    pub fn start_direct(&mut self, index: M) {
        self.release_current();
        self.index = index;
    }

    /// `reserve` -> `fill` -> `commit`.  Refused without a pool and while a batch is submitted.  Whatever fails after `reserve`, the
    /// slot goes back and nothing is pending.
    pub fn submit<F: FnOnce(&mut BatchSlot) -> Result<()>>(&mut self, kind: i32, param: i32, n_chains: usize, units: usize, index: M, fill: F) -> Result<()> {
        self.submit_io(kind, param, n_chains, units, 0, index, fill)
    }

    /// Does the pool narrow (`Pool::narrow_input`)?  `false` without a pool.
    pub fn narrow_input(&self) -> bool {
        match &self.pool {
            Some(pool) => pool.narrow_input(),
            None => false,
        }
    }

    /// The pool's input mode (`Pool::input_mode`).  0 without a pool.
    pub fn input_mode(&self) -> u8 {
        match &self.pool {
            Some(pool) => pool.input_mode(),
            None => 0,
        }
    }

    /// `submit` with an input format (`Pool::reserve_io`): `fill` writes plane 0 as `i16` words when `in_fmt` is `SYMACCEL_FMT_S16`.
    pub fn submit_io<F: FnOnce(&mut BatchSlot) -> Result<()>>(&mut self, kind: i32, param: i32, n_chains: usize, units: usize, in_fmt: i32, index: M, fill: F) -> Result<()> {
        let Some(pool) = self.pool.clone() else {
            return unsupported_error("no batcher");
        };
        if self.next.is_some() {
            return unsupported_error("one batch at a time");
        }
        let mut slot = pool.reserve_io(kind, param, n_chains, units, in_fmt)?;
        let filled = match fill(&mut slot) {
            Ok(()) => pool.commit(&mut slot),
            Err(e) => Err(e),
        };
        if let Err(e) = filled {
            pool.release(slot);
            return Err(e);
        }
        self.next = Some((slot, index));
        Ok(())
    }

    /// Wait for the submitted batch.  On error its slot goes back and the current batch stays current.  On success `read_back` sees the
    /// slot (its state planes hold the state after the batch), the old current slot goes back, the new one and its index are current.
    pub fn collect<F: FnOnce(&mut BatchSlot)>(&mut self, read_back: F) -> Result<()> {
        let (Some(pool), Some((mut slot, index))) = (self.pool.clone(), self.next.take()) else {
            return unsupported_error("nothing was submitted");
        };
        let status = pool.wait_raw(&mut slot);
        if status < 0 {
            // (back BEFORE the status is judged: INVALID_ARG is the panic class of `check`, and a panic must not keep a slot either)
            pool.release(slot);
            return pool.check(status);
        }
        read_back(&mut slot);
        self.release_current();
        self.cur = Some(slot);
        self.index = index;
        Ok(())
    }

    /// "Results will be wanted soon" (`Pool::hint`).
    pub fn hint(&self) {
        if let Some(pool) = &self.pool {
            pool.hint();
        }
    }

    /// Drop the submitted batch unseen.
    pub fn abandon(&mut self) {
        if let (Some(pool), Some((slot, _))) = (self.pool.clone(), self.next.take()) {
            pool.release(slot);
        }
    }

    fn release_current(&mut self) {
        if let (Some(pool), Some(slot)) = (self.pool.clone(), self.cur.take()) {
            pool.release(slot);
        }
    }

    /// Both slots go back: what `Drop` does.
    pub fn release_all(&mut self) {
        self.abandon();
        self.release_current();
    }
}

impl<M> Drop for SlotCycle<M> {
    fn drop(&mut self) {
        self.release_all();
    }
}

/// One plane of a batch in the packet-major layout that the FLAC and ALAC entry points and their batcher slots share: row `i * nch + c`
/// of `dst` (rows of `pitch` elements) is channel `c` of packet `i`'s plane, `zero` behind a shorter one.
pub(crate) fn place_rows<P, T: Copy>(dst: &mut [T], batch: &[P], nch: usize, pitch: usize, zero: T, plane: impl Fn(&P) -> &[T]) {
    for (i, p) in batch.iter().enumerate() {
        let src = plane(p);
        let w = src.len() / nch;
        for c in 0..nch {
            let at = (i * nch + c) * pitch;
            dst[at..at + w].copy_from_slice(&src[c * w..(c + 1) * w]);
            dst[at + w..at + pitch].fill(zero);
        }
    }
}

/// The words of every packet of a batch as `i16`, if every one of them fits: one `symaccel_host_narrow_s16` per packet decides and packs
/// in the same pass.  `None` as soon as a packet has a word that does not fit (a side channel's 17-bit warm-up): the batch goes up wide.
pub(crate) fn narrow_words<P>(batch: &[P], words: impl Fn(&P) -> &[i32]) -> Option<Vec<Vec<i16>>> {
    let mut packed: Vec<Vec<i16>> = Vec::with_capacity(batch.len());
    for p in batch.iter() {
        let src = words(p);
        let mut dst = vec![0i16; src.len()];
        // SAFETY: `src` and `dst` hold `src.len()` words each; plain host code.
        if unsafe { ffi::symaccel_host_narrow_s16(src.as_ptr(), dst.as_mut_ptr(), src.len()) } == 0 {
            return None;
        }
        packed.push(dst);
    }
    Some(packed)
}

/// The rows of a batch for `SYMACCEL_IN_FMT_ROWS`: row `i * nch + c` is channel `c` of packet `i`, packed at the narrowest of 2, 3 or 4
/// bytes a word that holds every word of it (`symaccel_host_pack_row` decides and packs), its width, and the rows per width.
pub(crate) struct PackedRows {
    pub rows: Vec<Vec<u8>>,
    pub widths: Vec<u8>,
    pub counts: [usize; 3],
}

/// No pass over the batch in front and no prefix sum: every row is packed on its own.  A 17-bit warm-up costs its row a third byte a
/// word, not the batch its narrow transport.
pub(crate) fn pack_rows<P>(batch: &[P], nch: usize, words: impl Fn(&P) -> &[i32]) -> PackedRows {
    let mut packed = PackedRows { rows: Vec::with_capacity(batch.len() * nch), widths: Vec::with_capacity(batch.len() * nch), counts: [0; 3] };
    for p in batch.iter() {
        let src = words(p);
        let w = src.len() / nch;
        for c in 0..nch {
            let row = &src[c * w..(c + 1) * w];
            let mut dst = vec![0u8; 4 * w];
            // SAFETY: `row` holds `w` words, `dst` the 4 * w bytes the widest packing takes; plain host code.
            let width = unsafe { ffi::symaccel_host_pack_row(row.as_ptr(), dst.as_mut_ptr() as *mut core::ffi::c_void, w) } as usize;
            dst.truncate(w * width);
            packed.counts[width - 2] += 1;
            packed.widths.push(width as u8);
            packed.rows.push(dst);
        }
    }
    packed
}

impl PackedRows {
    /// Into plane 0 of a slot whose rows are `pitch` words apart: row `r` starts where it starts in the native plane, at byte
    /// `r * pitch * 4`; zero words at the row's width behind a shorter one.  The bytes of the row's region behind that are not read.
    pub fn place(&self, dst: &mut [u8], pitch: usize) {
        for (r, row) in self.rows.iter().enumerate() {
            let at = r * pitch * 4;
            dst[at..at + row.len()].copy_from_slice(row);
            dst[at + row.len()..at + pitch * self.widths[r] as usize].fill(0);
        }
    }
}

/// Page-locked host memory (symaccel_host_alloc): what the staged host entry points need to overlap H2D, kernels and D2H.
pub struct Pinned<T: Copy> {
    ptr: *mut T,
    len: usize,
}

unsafe impl<T: Copy + Send> Send for Pinned<T> {}
unsafe impl<T: Copy + Sync> Sync for Pinned<T> {}

impl<T: Copy + Default> Pinned<T> {
    pub fn new(len: usize) -> Result<Self> {
        let mut p: *mut core::ffi::c_void = ptr::null_mut();
        // SAFETY: valid out-pointer; the allocation is released in Drop.
        check(unsafe { ffi::symaccel_host_alloc(len.max(1) * std::mem::size_of::<T>(), &mut p) }, ptr::null())?;
        let ptr = p as *mut T;
        for i in 0..len {
            // SAFETY: inside the allocation.
            unsafe { ptr.add(i).write(T::default()) };
        }
        Ok(Pinned { ptr, len })
    }
}

impl<T: Copy> Pinned<T> {
    pub fn as_slice(&self) -> &[T] {
        // SAFETY: `len` initialised elements.
        unsafe { std::slice::from_raw_parts(self.ptr, self.len) }
    }

    pub fn as_mut_slice(&mut self) -> &mut [T] {
        // SAFETY: unique access through &mut self.
        unsafe { std::slice::from_raw_parts_mut(self.ptr, self.len) }
    }
}

impl<T: Copy> Drop for Pinned<T> {
    fn drop(&mut self) {
        // SAFETY: allocated by symaccel_host_alloc.
        unsafe { ffi::symaccel_host_free(self.ptr as *mut core::ffi::c_void) };
    }
}
