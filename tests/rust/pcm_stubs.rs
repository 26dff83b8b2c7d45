// TEST ONLY.  The twenty PCM codec ids (symphonia-core/src/codecs/audio.rs, well_known), beside tests/rust/audio_stubs.rs and
// tests/rust/adpcm_stubs.rs, which hold the ids of the codecs that came before.
pub const CODEC_ID_PCM_S32LE: AudioCodecId = AudioCodecId(0x100);
pub const CODEC_ID_PCM_S32BE: AudioCodecId = AudioCodecId(0x102);
pub const CODEC_ID_PCM_S24LE: AudioCodecId = AudioCodecId(0x104);
pub const CODEC_ID_PCM_S24BE: AudioCodecId = AudioCodecId(0x106);
pub const CODEC_ID_PCM_S16LE: AudioCodecId = AudioCodecId(0x108);
pub const CODEC_ID_PCM_S16BE: AudioCodecId = AudioCodecId(0x10a);
pub const CODEC_ID_PCM_S8: AudioCodecId = AudioCodecId(0x10c);
pub const CODEC_ID_PCM_U32LE: AudioCodecId = AudioCodecId(0x10e);
pub const CODEC_ID_PCM_U32BE: AudioCodecId = AudioCodecId(0x110);
pub const CODEC_ID_PCM_U24LE: AudioCodecId = AudioCodecId(0x112);
pub const CODEC_ID_PCM_U24BE: AudioCodecId = AudioCodecId(0x114);
pub const CODEC_ID_PCM_U16LE: AudioCodecId = AudioCodecId(0x116);
pub const CODEC_ID_PCM_U16BE: AudioCodecId = AudioCodecId(0x118);
pub const CODEC_ID_PCM_U8: AudioCodecId = AudioCodecId(0x11a);
pub const CODEC_ID_PCM_F32LE: AudioCodecId = AudioCodecId(0x11c);
pub const CODEC_ID_PCM_F32BE: AudioCodecId = AudioCodecId(0x11e);
pub const CODEC_ID_PCM_F64LE: AudioCodecId = AudioCodecId(0x120);
pub const CODEC_ID_PCM_F64BE: AudioCodecId = AudioCodecId(0x122);
pub const CODEC_ID_PCM_ALAW: AudioCodecId = AudioCodecId(0x124);
pub const CODEC_ID_PCM_MULAW: AudioCodecId = AudioCodecId(0x125);

// Stand-ins for what PcmDecoder (symphonia-codec-pcm/src/lib.rs) needs of symphonia-core's containers beyond tests/rust/audio_stubs.rs, so
// that the reference's `PcmDecoder::try_new` and `decode_ref` can be EXECUTED under tools/rsinterp (tools/make_pcm_decode_fixtures.py).
// Same names and signatures as the reference; the bodies are the reference's logic without SmallVec and MutableAudioPlaneSlices.
// Everything that reads or computes a sample -- io/, audio/sample.rs, audio/conv.rs, lib.rs -- is the reference's own text.

/// audio/buf.rs:318-346 (render_with: frame by frame, a frame is committed only if the render function returned Ok; with `None` the
/// remaining capacity is rendered) and audio/buf.rs grow_capacity (never shrinks)
impl<S> AudioBuffer<S> {
    pub fn render_with<F>(&mut self, num_frames: Option<usize>, mut f: F) -> Result<usize> {
        let num_new_frames = num_frames.unwrap_or(self.capacity - self.num_frames);
        let end = self.num_frames + num_new_frames;
        assert!(end <= self.capacity, "capacity will be exceeded");
        while self.num_frames < end {
            f(self.num_frames, &mut self.planes)?;
            self.num_frames += 1;
        }
        Ok(num_new_frames - (end - self.num_frames))
    }
    pub fn grow_capacity(&mut self, new_capacity: usize) {
        if new_capacity > self.capacity {
            for plane in &mut self.planes {
                while plane.len() < new_capacity {
                    plane.push(audio_stub_sample_mid());
                }
            }
            self.capacity = new_capacity;
        }
    }
}

/// audio/generic.rs: one variant per sample format, each method forwarding to the buffer it holds
pub enum GenericAudioBuffer {
    U8(AudioBuffer<u8>),
    U16(AudioBuffer<u16>),
    U24(AudioBuffer<u24>),
    U32(AudioBuffer<u32>),
    S8(AudioBuffer<i8>),
    S16(AudioBuffer<i16>),
    S24(AudioBuffer<i24>),
    S32(AudioBuffer<i32>),
    F32(AudioBuffer<f32>),
    F64(AudioBuffer<f64>),
}

impl GenericAudioBuffer {
    pub fn new(format: SampleFormat, spec: AudioSpec, capacity: usize) -> Self {
        match format {
            SampleFormat::U8 => GenericAudioBuffer::U8(AudioBuffer::new(spec, capacity)),
            SampleFormat::U16 => GenericAudioBuffer::U16(AudioBuffer::new(spec, capacity)),
            SampleFormat::U24 => GenericAudioBuffer::U24(AudioBuffer::new(spec, capacity)),
            SampleFormat::U32 => GenericAudioBuffer::U32(AudioBuffer::new(spec, capacity)),
            SampleFormat::S8 => GenericAudioBuffer::S8(AudioBuffer::new(spec, capacity)),
            SampleFormat::S16 => GenericAudioBuffer::S16(AudioBuffer::new(spec, capacity)),
            SampleFormat::S24 => GenericAudioBuffer::S24(AudioBuffer::new(spec, capacity)),
            SampleFormat::S32 => GenericAudioBuffer::S32(AudioBuffer::new(spec, capacity)),
            SampleFormat::F32 => GenericAudioBuffer::F32(AudioBuffer::new(spec, capacity)),
            SampleFormat::F64 => GenericAudioBuffer::F64(AudioBuffer::new(spec, capacity)),
        }
    }
    pub fn clear(&mut self) {
        match self {
            GenericAudioBuffer::U8(buf) => buf.clear(),
            GenericAudioBuffer::U16(buf) => buf.clear(),
            GenericAudioBuffer::U24(buf) => buf.clear(),
            GenericAudioBuffer::U32(buf) => buf.clear(),
            GenericAudioBuffer::S8(buf) => buf.clear(),
            GenericAudioBuffer::S16(buf) => buf.clear(),
            GenericAudioBuffer::S24(buf) => buf.clear(),
            GenericAudioBuffer::S32(buf) => buf.clear(),
            GenericAudioBuffer::F32(buf) => buf.clear(),
            GenericAudioBuffer::F64(buf) => buf.clear(),
        }
    }
    pub fn grow_capacity(&mut self, new_capacity: usize) {
        match self {
            GenericAudioBuffer::U8(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::U16(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::U24(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::U32(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::S8(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::S16(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::S24(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::S32(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::F32(buf) => buf.grow_capacity(new_capacity),
            GenericAudioBuffer::F64(buf) => buf.grow_capacity(new_capacity),
        }
    }
    /// (the reference hands out a GenericAudioBufferRef of the same variant over the same buffer: the stand-in is its own reference)
    pub fn as_generic_audio_buffer_ref(&self) -> &GenericAudioBuffer {
        self
    }
}

/// `(read << shift).into_sample()` of lib.rs:58, 76: `IntoSample<T>` for `F` is `T::from_sample(self)` (audio/conv.rs:632-637) with `T` the
/// sample type of the buffer the macro matched.  The interpreter does not track the type an expression is assigned to, so the fixture
/// generator rewrites that one call, in memory, into this function with the macro's own `$fmt` as the first argument.
pub fn pcm_stub_into_sample<F>(format: SampleFormat, sample: F) {
    match format {
        SampleFormat::U8 => u8::from_sample(sample),
        SampleFormat::U16 => u16::from_sample(sample),
        SampleFormat::U24 => u24::from_sample(sample),
        SampleFormat::U32 => u32::from_sample(sample),
        SampleFormat::S8 => i8::from_sample(sample),
        SampleFormat::S16 => i16::from_sample(sample),
        SampleFormat::S24 => i24::from_sample(sample),
        SampleFormat::S32 => i32::from_sample(sample),
        SampleFormat::F32 => f32::from_sample(sample),
        SampleFormat::F64 => f64::from_sample(sample),
    }
}
