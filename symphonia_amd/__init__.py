"""symphonia_amd -- MI355X-native batched synthesis backend for Symphonia's DSP hot path.

The compute lives in symphonia_amd/libsymaccel.so (hand-written HIP for gfx950 behind the C ABI
of include/symaccel.h).  This package is the thin host-side mirror of the reference's interfaces.
There is no CPU fallback: importing works anywhere, creating a Context needs the library + a GPU.
"""
from ._ffi import Library, SymaccelError, default_library  # noqa: F401
from .backend import (PinnedBuffer, Batcher, BatchSlot, BATCH_AAC_SYNTH, BATCH_MP3_SYNTH, BATCH_MP3_DECODE, BATCH_VORBIS_SYNTH, BATCH_AAC_DECODE, BATCH_VORBIS_DECODE, BATCH_FLAC_RESTORE, BATCH_ALAC_PREDICT, BATCH_ADPCM_DECODE, BATCH_MPA12_DECODE, BATCH_PCM_DECODE, AAC_PULSE_DTYPE, aac_pulse, vorbis_bark_map, vorbis_floor0_coeffs, vorbis_floor0, flac_block_status, alac_block_status, vorbis_floor1_status, aac_tns_status,  # noqa: F401
                      AacDsp, AacSpectralTools, VORBIS_FLOOR1_DTYPE, AAC_JS_DTYPE, AAC_TNS_DTYPE, AAC_JS_MS, AAC_JS_INTENSITY, AlacPredictor, Context, Fft, FlacPredictor, Ifft, Imdct, Mp3Requantize, Mp3Stereo, Mp3Synthesis, MpaPolyphase, VorbisDsp,  # noqa: F401
                      MP3_REQUANT_DTYPE, MP3_RQ_PREFLAG, MP3_RQ_SCALEFAC_SCALE, MP3_STEREO_DTYPE, MP3_ST_MID_SIDE, MP3_ST_INTENSITY,
                      MP3_ST_MPEG1, MP3_ST_IS_SCALE,
                      aac_side, alac_desc, flac_desc, mp3_side, FLAC_FIXED, FLAC_LPC, FLAC_VERBATIM,
                      MD5_STATE_DTYPE, FLAC_MD5_FRAME_DTYPE, FLAC_MD5_JOB_DTYPE, flac_bytes_per_sample, md5_init, md5_update, md5_digest, flac_md5_frames, flac_md5,
                      flac_md5_device, flac_md5_finish_device,
                      FMT_U8, FMT_S8, FMT_U16, FMT_S16, FMT_U24, FMT_S24, FMT_U32, FMT_S32, FMT_F32, SAMPLE_FORMATS, sample_format, sample_bytes, pcm_convert, IN_FMT_ROWS, input_format, host_pack_row,
                      pcm_convert_device,
                      ADPCM_MS, ADPCM_IMA_WAV, ADPCM_IMA_QT, ADPCM_CODECS, adpcm_codec, adpcm_block_bytes, adpcm_decode, adpcm_decode_device,
                      MPA_LAYER1, MPA_LAYER2, Mpa12Decode,
                      PCM_S32LE, PCM_S32BE, PCM_S24LE, PCM_S24BE, PCM_S16LE, PCM_S16BE, PCM_S8, PCM_U32LE, PCM_U32BE, PCM_U24LE, PCM_U24BE, PCM_U16LE,
                      PCM_U16BE, PCM_U8, PCM_F32LE, PCM_F32BE, PCM_F64LE, PCM_F64BE, PCM_ALAW, PCM_MULAW, PCM_CODECS, pcm_codec, pcm_native_dtype,
                      pcm_coded_bytes, pcm_native_bytes, pcm_decode, pcm_decode_device)

__all__ = ["Library", "SymaccelError", "default_library", "Context", "Imdct", "Fft", "Ifft", "AacDsp", "AacSpectralTools", "Mp3Synthesis", "Mp3Requantize", "Mp3Stereo", "MpaPolyphase", "Mpa12Decode",
           "VorbisDsp", "FlacPredictor", "AlacPredictor", "aac_side", "mp3_side", "flac_desc", "alac_desc"]
