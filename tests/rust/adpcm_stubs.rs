// TEST ONLY.  The three ADPCM codec ids (symphonia-core/src/codecs/audio.rs, well_known), beside tests/rust/audio_stubs.rs, which holds the
// ids of the five codecs that came before.
pub const CODEC_ID_ADPCM_MS: AudioCodecId = AudioCodecId(0x203);
pub const CODEC_ID_ADPCM_IMA_WAV: AudioCodecId = AudioCodecId(0x204);
pub const CODEC_ID_ADPCM_IMA_QT: AudioCodecId = AudioCodecId(0x205);
