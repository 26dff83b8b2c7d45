// TEST ONLY.  A stand-in for `rand::rngs::SmallRng`, for the two `fuzz_bitstream*_read_codebook` tests of symphonia-core's io/bit.rs
// when tests/test_reference_unit_tests.py runs them under tools/rsinterp (the `rand` crate is not part of the reference tree).
//
// It does NOT reproduce the rand crate's stream: this is SplitMix64 (Steele, Lea, Flood 2014; public domain constants).  The two
// tests do not depend on the stream -- what they assert (`bs.buf.len() == 0` once `read_codebook` stops returning Ok) must hold for
// any 64 bytes -- so any generator that fills the buffer with well-mixed bytes exercises the same property.  Only the two calls
// the tests make are provided: `SmallRng::seed_from_u64` (rand::SeedableRng) and `fill_bytes` (rand::RngCore).

pub struct SmallRng {
    state: u64,
}

impl SmallRng {
    pub fn seed_from_u64(seed: u64) -> SmallRng {
        SmallRng { state: seed }
    }

    pub fn next_u64(&mut self) -> u64 {
        self.state = self.state.wrapping_add(0x9e37_79b9_7f4a_7c15);
        let mut z = self.state;
        z = (z ^ (z >> 30)).wrapping_mul(0xbf58_476d_1ce4_e5b9);
        z = (z ^ (z >> 27)).wrapping_mul(0x94d0_49bb_1331_11eb);
        z ^ (z >> 31)
    }

    pub fn fill_bytes(&mut self, dest: &mut [u8]) {
        let mut i = 0;
        while i < dest.len() {
            let word = self.next_u64().to_le_bytes();
            let mut k = 0;
            while k < 8 && i < dest.len() {
                dest[i] = word[k];
                i += 1;
                k += 1;
            }
        }
    }
}
