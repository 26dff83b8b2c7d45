// A scripted FLAC front end that also answers `expected_md5` (tests/test_rust_flac_verify.py): what SeamFrontEnd reads out of
// STREAMINFO, here a field of the script.
pub struct VerifiedFlacFront {
    pub params: AudioCodecParameters,
    pub nch: usize,
    pub max_bs: usize,
    pub script: Vec<ParsedFlac>,
    pub parses: usize,
    pub md5: Option<[u8; 16]>,
}

impl FlacFrontEnd for VerifiedFlacFront {
    fn params(&self) -> &AudioCodecParameters {
        &self.params
    }
    fn channels(&self) -> usize {
        self.nch
    }
    fn max_blocksize(&self) -> usize {
        self.max_bs
    }
    fn expected_md5(&self) -> Option<[u8; 16]> {
        self.md5
    }
    fn parse(&mut self, packet: &PacketRef<'_>) -> Result<ParsedFlac> {
        let i = script_index(packet)?;
        self.parses += 1;
        let p = &self.script[i];
        Ok(ParsedFlac {
            blocksize: p.blocksize,
            words: p.words.clone(),
            desc: p.desc.clone(),
            coeffs: p.coeffs.clone(),
            pair_mode: p.pair_mode,
            out_shift: p.out_shift,
        })
    }
}
