// csm_webpdec.h -- the lossless WebP decoder's kernels (webpdec.hip) as the library's other files launch them: the lossy decoder
// (webplossy.hip) decodes the alpha planes of its files with them.  Host side, inside libcsm355 only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace csm {

// desc_host: the [n][12] descriptors of csm_webp_decode.  planes: every descriptor is an alpha plane -- word [6] is 1, word [3]
// (channels) is 1, the input is a VP8L stream without its 5-byte header, and the output is the green channel, one byte per pixel.
size_t vp8l_scratch_bytes(const int32_t *desc_host, int n, bool planes);
// the walk, the inverse transforms and the store, enqueued on the stream; nothing is waited for
int vp8l_launch(const uint8_t *blob, int64_t blob_bytes, const int32_t *desc_host, int n, uint8_t *out, int64_t out_bytes, void *scratch,
                bool planes, hipStream_t st);
// the error word of every file of a launch over `scratch` (csm_vp8l.h); waits for the stream
int vp8l_errors(const void *scratch, int n, uint32_t *err_host, hipStream_t st);

}  // namespace csm
