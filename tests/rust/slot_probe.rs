//! TEST ONLY.  The smallest codec `SlotCycle` (bindings/rust/symphonia-accel-hip/src/ctx.rs) can be driven with under tools/rsinterp
//! (tests/test_rust_slots.py): batcher kind 10, Layer I, one chain, one packet -- 384 codes and a 64-byte record in, 384 samples out,
//! `vvec[1024]` / `vfront[1]` carried from batch to batch.  The index of a batch is a tag the test gives it.

pub struct SlotProbe {
    pub slots: SlotCycle<i64>,
    pub vvec: Vec<f32>,
    pub vfront: Vec<i32>,
}

impl SlotProbe {
    pub fn new_pooled() -> Result<SlotProbe> {
        Ok(SlotProbe { slots: SlotCycle::new(Some(Pool::shared()?), -1), vvec: vec![0.0; 1024], vfront: vec![0; 1] })
    }

    /// `fail_fill`: the fill gives up before it has written anything, as a codec whose batch does not fit its slot does.
    pub fn submit(&mut self, tag: i64, codes: &[u16], rec: &[u8], fail_fill: bool) -> Result<()> {
        self.slots.submit(ffi::SYMACCEL_BATCH_MPA12_DECODE as i32, ffi::SYMACCEL_MPA_LAYER1 as i32, 1, 1, tag, |slot| {
            if fail_fill {
                return decode_error("probe: the fill failed");
            }
            slot.input::<u16>(0)[..384].copy_from_slice(codes);
            slot.input::<u8>(1)[..64].copy_from_slice(rec);
            slot.state::<f32>(0)[..1024].copy_from_slice(&self.vvec);
            slot.state::<i32>(1)[..1].copy_from_slice(&self.vfront);
            Ok(())
        })
    }

    pub fn collect(&mut self) -> Result<()> {
        self.slots.collect(|slot| {
            self.vvec.copy_from_slice(&slot.state::<f32>(0)[..1024]);
            self.vfront.copy_from_slice(&slot.state::<i32>(1)[..1]);
        })
    }

    pub fn abandon(&mut self) {
        self.slots.abandon();
    }

    pub fn start_direct(&mut self, tag: i64) {
        self.slots.start_direct(tag);
    }

    pub fn release_all(&mut self) {
        self.slots.release_all();
    }

    pub fn tag(&self) -> i64 {
        *self.slots.index()
    }

    /// What `publish` would read: the PCM of the current batch in its slot (copied out for the test), `None` without a slot.
    pub fn out(&self) -> Option<Vec<f32>> {
        match self.slots.out::<f32>() {
            Some(pcm) => Some(pcm[..384].to_vec()),
            None => None,
        }
    }
}
