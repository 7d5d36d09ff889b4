// flm_gemv4.h -- W4A8 (FLM_QT_INT4): the weight formats around the nibble GEMV and the kernels that convert between them.  Part of flm_kernels.h; the GEMV itself is
// k_gemv<QT_INT4, ..> (flm_gemv.h: the GemvCtx branches marked W4).
//
// INTERCHANGE format (the reference's Bit4Pair: what flm_upload_tensor, flm_op_matmul_q and flm_op_quantize exchange with the host): a row of `cols` weights is cols / 2
// bytes, element 2i in the low nibble and element 2i + 1 in the high nibble of byte i, two's complement in [-8, 7]; fp32 scales [rows][cols / 64].
//
// DEVICE layout (what every kernel streams; made once at upload, in place): the same bytes per row, and inside every 32-bit word of 8 consecutive weights e0 .. e7
//     byte j = u_j | u_{j+4} << 4,   u = q + 8 = q ^ 8 in 0 .. 15
// so that  w & 0x0F0F0F0F  is the four bytes u0 .. u3 -- next to the activation's dword of the same four columns -- and  (w >> 4) & 0x0F0F0F0F  is u4 .. u7, next to the
// following dword: no per-byte shift, no sign extension, and bytes 0 .. 15 are valid signed operands of v_dot4_i32_i8.  The offset leaves once per quant group, exactly:
//     sum (u - 8) x = sum u x - 8 sum x
// with sum x the activation's per-group int32 sum, computed where the activation is quantized (gemv_prologue) and kept in LDS next to its scales.  All three terms are exact
// int32 values, so the float the group leader parks is the one the int8 kernel parks for the sign-extended nibbles, and the fp32 chain behind it is the int8 kernel's.
// Both conversions are word-local: a word of the interchange format holds the same 8 weights as the word of the device layout at the same place.
#pragma once
#include "flm_math.h"
#pragma clang fp contract(off)

namespace flm {

// interchange word (nibble i = e_i, signed) -> device word
__device__ __forceinline__ uint32_t w4_word_to_device(uint32_t v) {
    v ^= 0x88888888u;                                                          // u = q ^ 8
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) o |= (((v >> (4 * j)) & 0xFu) | (((v >> (4 * j + 16)) & 0xFu) << 4)) << (8 * j);
    return o;
}

// in place over the words of a packed matrix (rows x cols / 8 of them)
inline __global__ void k_repack_w4(uint32_t* w, size_t nwords) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += stride) w[i] = w4_word_to_device(w[i]);
}

// The project's quantizer with F = 7 over a flat fp32 array (the third case of k_quantize_flat, flm_gpu.hip): r = max|x| / 7, q = trunc(x / r), an all-zero group r = 0, q = 0;
// 16 lanes own a 64-group, a lane's four values are two bytes of the INTERCHANGE format
__device__ __forceinline__ void quantize4_store(void* q, size_t e, int q0, int q1, int q2, int q3) {
    reinterpret_cast<uint16_t*>(q)[e / 4] = (uint16_t)((q0 & 0xF) | ((q1 & 0xF) << 4) | ((q2 & 0xF) << 8) | ((q3 & 0xF) << 12));
}

} // namespace flm
