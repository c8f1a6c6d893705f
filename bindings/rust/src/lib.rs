//! UNVERIFIED (no Rust toolchain in the build image).  Drop-in module tree for callers of density-rs 0.16.6 that routes the
//! encode/decode path to libdensity_hip.so.  Paths, names and signatures follow the reference:
//!   density_rs::algorithms::chameleon::chameleon::Chameleon::{encode, decode}   (src/algorithms/chameleon/chameleon.rs:45-53)
//!   density_rs::codec::codec::Codec::safe_encode_buffer_size                    (src/codec/codec.rs:18-21)
//!   density_rs::errors::{encode_error::EncodeError, decode_error::DecodeError}  (src/errors/*.rs)

#[link(name = "density_hip")]
extern "C" {
    // include/density_hip.h section 1 == src/algorithms/chameleon/chameleon.rs:70-83 (and cheetah.rs:105-118, lion.rs:193-206)
    fn chameleon_encode(input: *const u8, input_size: usize, output: *mut u8, output_size: usize) -> usize;
    fn chameleon_decode(input: *const u8, input_size: usize, output: *mut u8, output_size: usize) -> usize;
    fn chameleon_safe_encode_buffer_size(size: usize) -> usize;
    fn cheetah_encode(input: *const u8, input_size: usize, output: *mut u8, output_size: usize) -> usize;
    fn cheetah_decode(input: *const u8, input_size: usize, output: *mut u8, output_size: usize) -> usize;
    fn cheetah_safe_encode_buffer_size(size: usize) -> usize;
    fn lion_encode(input: *const u8, input_size: usize, output: *mut u8, output_size: usize) -> usize;
    fn lion_decode(input: *const u8, input_size: usize, output: *mut u8, output_size: usize) -> usize;
    fn lion_safe_encode_buffer_size(size: usize) -> usize;
}

/// include/density_hip.h section 2, sealed containers (DENSITY_HIP_FLAG_CHECKSUM): what a CPU reader and a host-pointer producer link.  The device-pointer calls
/// (density_hip_checksum_device, density_hip_seal_device, density_hip_decode_device_verdicts, density_hip_parity_device, density_hip_parity_update_device, density_hip_decode_device_recover) take a hipStream_t and belong to a caller that already binds HIP; they are declared here in step with the header.
pub mod sealed {
    pub const DENSITY_HIP_FLAG_CHECKSUM: u16 = 8;
    pub const DENSITY_HIP_ERR_CHECKSUM: i32 = 6;
    pub const DENSITY_HIP_CHUNK_DAMAGED: u32 = 1;
    pub const DENSITY_HIP_SALVAGE_BLANK: u32 = 1;
    pub const DENSITY_HIP_CHUNK_RECOVERED: u32 = 2;
    pub const DENSITY_HIP_PARITY_MAGIC: u32 = 0x31504844;
    #[repr(C)]
    pub struct DensityHipHeader { pub magic: u32, pub algo: u8, pub version: u8, pub flags: u16, pub chunk_size: u32, pub n_chunks: u32, pub total_len: u64, pub container_len: u64 }
    /// the first 32 bytes of a parity blob "DHP1": n_groups rows of row_bytes bytes follow, row g the XOR of the input chunks i with i % n_groups == g
    #[repr(C)]
    pub struct DensityHipParityHeader { pub magic: u32, pub version: u8, pub reserved0: u8, pub reserved1: u16, pub chunk_size: u32, pub n_chunks: u32, pub total_len: u64,
                                        pub n_groups: u32, pub row_bytes: u32 }
    #[link(name = "density_hip")]
    extern "C" {
        /// C of one decoded chunk, host arithmetic (no device): compare with trailer entry i at container_len - round_up(4 * n_chunks, 16) + 4 * i
        pub fn density_hip_checksum32(data: *const u8, size: usize) -> u32;
        pub fn density_hip_seal_overhead(input_size: usize, chunk_size: usize) -> usize;
        pub fn density_hip_encode_sealed(algo: i32, input: *const u8, input_size: usize, output: *mut u8, output_size: usize, chunk_size: usize) -> usize;
        pub fn density_hip_checksum_device(d_data: *const core::ffi::c_void, size: usize, chunk_size: usize, d_sums: *mut u32, stream: *mut core::ffi::c_void) -> i32;
        pub fn density_hip_seal_device(d_input: *const core::ffi::c_void, input_size: usize, d_container: *mut core::ffi::c_void, container_capacity: usize,
                                       header: *const DensityHipHeader, stream: *mut core::ffi::c_void, header_out: *mut DensityHipHeader) -> i32;
        /// verdicts and salvage: a word per chunk (0 = the chunk's bytes in the output have the trailer's checksum, DENSITY_HIP_CHUNK_DAMAGED otherwise), the output kept;
        /// flags: DENSITY_HIP_SALVAGE_BLANK zeroes the damaged chunks' bytes.  d_verdicts: device; verdicts and damaged_out: host.
        pub fn density_hip_decode_device_verdicts(d_container: *const core::ffi::c_void, container_size: usize, header: *const DensityHipHeader, d_output: *mut core::ffi::c_void,
                                                  output_capacity: usize, d_workspace: *mut core::ffi::c_void, workspace_size: usize, stream: *mut core::ffi::c_void,
                                                  d_verdicts: *mut u32, flags: core::ffi::c_uint, damaged_out: *mut u32) -> i32;
        pub fn density_hip_decode_verdicts(container: *const u8, container_size: usize, output: *mut u8, output_size: usize, verdicts: *mut u32,
                                           verdict_capacity: usize, flags: core::ffi::c_uint, damaged_out: *mut u32) -> usize;
        /// recovery records: the parity blob of an input (a sidecar: no container holds it), and the verdict decode that rebuilds every chunk that is the only
        /// damaged one of its group (verdict DENSITY_HIP_CHUNK_RECOVERED); d_parity: device; parity_header, damaged_out, recovered_out: host, each optional.
        pub fn density_hip_parity_size(input_size: usize, chunk_size: usize, n_groups: u32) -> usize;
        pub fn density_hip_parity_device(d_input: *const core::ffi::c_void, input_size: usize, chunk_size: usize, n_groups: u32, d_parity: *mut core::ffi::c_void,
                                         parity_capacity: usize, stream: *mut core::ffi::c_void) -> i32;
        pub fn density_hip_parity(input: *const u8, input_size: usize, chunk_size: usize, n_groups: u32, parity: *mut u8, parity_capacity: usize) -> usize;
        /// version 2 of the blob: Q rows over GF(2^8) behind the P rows, so that any two damaged chunks of a group (of at most 255) are rebuilt
        pub fn density_hip_parity2_size(input_size: usize, chunk_size: usize, n_groups: u32) -> usize;
        pub fn density_hip_parity2_device(d_input: *const core::ffi::c_void, input_size: usize, chunk_size: usize, n_groups: u32, d_parity: *mut core::ffi::c_void,
                                          parity_capacity: usize, stream: *mut core::ffi::c_void) -> i32;
        pub fn density_hip_parity2(input: *const u8, input_size: usize, chunk_size: usize, n_groups: u32, parity: *mut u8, parity_capacity: usize) -> usize;
        /// parity update: the blob at d_parity kept current after input bytes [offset, offset + old_size) changed from d_old to d_new (a same-size edit, or one
        /// of the tail: append, truncation); only the rows of the edited chunks are touched.  parity_header, header_out: host, each optional.
        pub fn density_hip_parity_update_header(header: *const DensityHipParityHeader, offset: u64, old_size: usize, new_size: usize,
                                                header_out: *mut DensityHipParityHeader) -> i32;
        pub fn density_hip_parity_update_device(d_parity: *mut core::ffi::c_void, parity_size: usize, parity_header: *const DensityHipParityHeader, offset: u64,
                                                d_old: *const core::ffi::c_void, old_size: usize, d_new: *const core::ffi::c_void, new_size: usize,
                                                stream: *mut core::ffi::c_void, header_out: *mut DensityHipParityHeader) -> i32;
        pub fn density_hip_parity_update(parity: *mut u8, parity_size: usize, offset: u64, old_data: *const u8, old_size: usize, new_data: *const u8,
                                         new_size: usize) -> usize;
        pub fn density_hip_decode_device_recover(d_container: *const core::ffi::c_void, container_size: usize, header: *const DensityHipHeader, d_parity: *const core::ffi::c_void,
                                                 parity_size: usize, parity_header: *const DensityHipParityHeader, d_output: *mut core::ffi::c_void, output_capacity: usize,
                                                 d_workspace: *mut core::ffi::c_void, workspace_size: usize, stream: *mut core::ffi::c_void, d_verdicts: *mut u32,
                                                 flags: core::ffi::c_uint, damaged_out: *mut u32, recovered_out: *mut u32) -> i32;
        pub fn density_hip_decode_recover(container: *const u8, container_size: usize, parity: *const u8, parity_size: usize, output: *mut u8, output_size: usize,
                                          verdicts: *mut u32, verdict_capacity: usize, flags: core::ffi::c_uint, damaged_out: *mut u32, recovered_out: *mut u32) -> usize;
    }
}

/// include/density_hip.h section 2, the container forms on the device: a PAGED container (sealed or not) to the packed wire form, byte for byte what
/// density_hip_encode_device (+ density_hip_seal_device) writes, a window of a container's chunks as a packed container of its own, and the windows of several
/// containers joined into one.  Device pointers and a
/// hipStream_t: for a caller that already binds HIP.
pub mod forms {
    pub use crate::sealed::DensityHipHeader;
    pub const DENSITY_HIP_FLAG_PAGED: u16 = 4;
    pub const DENSITY_HIP_JOIN_MAX_PARTS: u32 = 64;
    /// density_hip_join_part_t: a window of one container's chunks; `header` is a HOST copy of the container's first 32 bytes, chunk_count == 0 skips the part
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct DensityHipJoinPart {
        pub container: *const core::ffi::c_void,
        pub container_size: usize,
        pub header: *const DensityHipHeader,
        pub first_chunk: u32,
        pub chunk_count: u32,
    }
    #[link(name = "density_hip")]
    extern "C" {
        pub fn density_hip_unpage_device(d_container: *const core::ffi::c_void, container_size: usize, header: *const DensityHipHeader, d_output: *mut core::ffi::c_void,
                                         output_capacity: usize, d_workspace: *mut core::ffi::c_void, workspace_size: usize, stream: *mut core::ffi::c_void,
                                         header_out: *mut DensityHipHeader) -> i32;
        /// chunks [first_chunk, first_chunk + chunk_count) of a container of any form as a packed container of their own; a byte range is
        /// density_hip_chunk_range, density_hip_slice_device, density_hip_decode_device and `skip` added to the output pointer
        pub fn density_hip_chunk_range(header: *const DensityHipHeader, offset: u64, length: u64, first_chunk: *mut u32, chunk_count: *mut u32, skip: *mut u64) -> i32;
        pub fn density_hip_slice_bound(header: *const DensityHipHeader, first_chunk: u32, chunk_count: u32) -> usize;
        pub fn density_hip_slice_device(d_container: *const core::ffi::c_void, container_size: usize, header: *const DensityHipHeader, first_chunk: u32, chunk_count: u32,
                                        d_output: *mut core::ffi::c_void, output_capacity: usize, d_workspace: *mut core::ffi::c_void, workspace_size: usize,
                                        stream: *mut core::ffi::c_void, header_out: *mut DensityHipHeader) -> i32;
        pub fn density_hip_slice(container: *const u8, container_size: usize, first_chunk: u32, chunk_count: u32, output: *mut u8, output_size: usize) -> usize;
        /// the chunk windows of several containers (any forms; alike in algorithm, chunk size, block index and seal) as ONE packed container: append, the
        /// replacement of single chunks, a multi-rank container's rows as one container
        pub fn density_hip_join_bound(parts: *const DensityHipJoinPart, n_parts: u32) -> usize;
        pub fn density_hip_join_workspace_size(n_parts: u32, n_chunks_out: u32) -> usize;
        pub fn density_hip_join_device(parts: *const DensityHipJoinPart, n_parts: u32, d_output: *mut core::ffi::c_void, output_capacity: usize,
                                       d_workspace: *mut core::ffi::c_void, workspace_size: usize, stream: *mut core::ffi::c_void, header_out: *mut DensityHipHeader) -> i32;
        pub fn density_hip_join(parts: *const DensityHipJoinPart, n_parts: u32, output: *mut u8, output_size: usize) -> usize;
    }
}

pub mod errors {
    pub mod encode_error { #[derive(Debug)] pub struct EncodeError {} }
    pub mod decode_error { #[derive(Debug)] pub struct DecodeError {} }
}

pub mod codec {
    pub mod codec {
        pub trait Codec {
            fn safe_encode_buffer_size(size: usize) -> usize;
        }
    }
}

macro_rules! algo {
    ($m:ident, $t:ident, $enc:ident, $dec:ident, $safe:ident) => {
        pub mod $m {
            pub mod $m {
                use crate::codec::codec::Codec;
                use crate::errors::decode_error::DecodeError;
                use crate::errors::encode_error::EncodeError;
                pub struct $t {}
                impl $t {
                    pub fn encode(input: &[u8], output: &mut [u8]) -> Result<usize, EncodeError> {
                        if input.is_empty() { return Ok(0); }
                        let n = unsafe { crate::$enc(input.as_ptr(), input.len(), output.as_mut_ptr(), output.len()) };
                        if n == 0 { Err(EncodeError {}) } else { Ok(n) }
                    }
                    pub fn decode(input: &[u8], output: &mut [u8]) -> Result<usize, DecodeError> {
                        if input.is_empty() { return Ok(0); }
                        let n = unsafe { crate::$dec(input.as_ptr(), input.len(), output.as_mut_ptr(), output.len()) };
                        if n == 0 { Err(DecodeError {}) } else { Ok(n) }
                    }
                }
                impl Codec for $t {
                    fn safe_encode_buffer_size(size: usize) -> usize { unsafe { crate::$safe(size) } }
                }
            }
        }
    };
}

pub mod algorithms {
    algo!(chameleon, Chameleon, chameleon_encode, chameleon_decode, chameleon_safe_encode_buffer_size);
    algo!(cheetah, Cheetah, cheetah_encode, cheetah_decode, cheetah_safe_encode_buffer_size);
    algo!(lion, Lion, lion_encode, lion_decode, lion_safe_encode_buffer_size);
}
