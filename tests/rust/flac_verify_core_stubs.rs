// What the stand-in AudioCodecParameters of audio_stubs.rs lacks for a VERIFIED FLAC stream (tests/test_flac_verify_packets.py): the
// verification code the decoder reads out of STREAMINFO (symphonia-core codecs/audio.rs: `VerificationCheck`, `with_verification_code`).
// The test gives its parameter records a `verification_check` field.
// (the reference's finalize() formats both digests only when debug logging is on, decoder.rs:283: it is off here)
macro_rules! log_enabled {
    ($level:expr) => {
        false
    };
}

pub enum VerificationCheck {
    Crc8(u8),
    Crc16([u8; 2]),
    Crc32([u8; 4]),
    Md5([u8; 16]),
    Other(&'static str),
}

impl AudioCodecParameters {
    pub fn with_verification_code(&mut self, code: VerificationCheck) -> &mut Self {
        self.verification_check = Some(code);
        self
    }
}
