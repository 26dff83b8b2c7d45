//! TEST ONLY.  A `SubbandBackend` (the second seam of bindings/rust/patches/symphonia-bundle-mp3.diff) that keeps every frame the patched
//! Layer I / Layer II decoders hand it, so that tests/test_mpa12_packets.py can compare what crosses the seam with what the writer put
//! into the packets.  It produces no PCM.

pub struct RecordingSubband {
    pub frames: Vec<SubbandFrame>,
    pub resets: usize,
}

impl RecordingSubband {
    pub fn new() -> Self {
        RecordingSubband { frames: Vec::new(), resets: 0 }
    }
}

impl SubbandBackend for RecordingSubband {
    fn decode_frame(&mut self, frame: &SubbandFrame, _out: &mut AudioBuffer<f32>) {
        self.frames.push(frame.clone());
    }

    fn reset(&mut self) {
        self.resets += 1;
    }
}

pub fn mpa12_recording_backend() -> Box<dyn SubbandBackend> {
    Box::new(RecordingSubband::new())
}

/// codecs/audio.rs well-known ids of the two layers (the stand-ins of audio_stubs.rs name Layer III alone)
pub const CODEC_ID_MP1: AudioCodecId = AudioCodecId(0x1001);
pub const CODEC_ID_MP2: AudioCodecId = AudioCodecId(0x1002);
