// w2xc_conv_batch.hip -- conv3x3_first_batch / conv3x3_last_batch: the W2XC_K_FIRST / W2XC_K_LAST launches of a multi-plane (RGB) chain -- and their uint8
// forms W2XC_K_FIRST_U8 / W2XC_K_LAST_U8 -- for `batch` images of identical geometry in one launch (w2xc_convert_planes_batch_device, the batched image
// calls).  The kernels are the bodies of conv3x3_first / conv3x3_last (w2xc_first_body.inc / w2xc_last_body.inc) with the batch hooks on: batch x ntiles
// tiles, image-major, the image of a tile on the 64-bit bases only.  Per tile the same loads, MFMAs and stores as the single-image launch: bit-identical.
// Three planes in (first) / three planes out (last) only: what the batched chain of w2xc_select.cpp asks for.
#include "w2xc_kernels.h"
#include "w2xc_device.h"
#include "w2xc_layout.h"

#ifndef FIRST_TPW
#define FIRST_TPW 4
#endif
#ifndef LAST_TPW
#define LAST_TPW 4
#endif

#define FLB_ONLY(...) __VA_ARGS__
#define FLB_SEL(b_, s_) b_

// (U8: d.in is the BYTES of image 0 and bd.in_bs the image stride in bytes)
template <int CIN, int NBT, bool PLANAR, bool U8>
__global__ void __launch_bounds__(256) conv3x3_first_batch(W2xcConvDesc d, int tiles_x, int ntiles, W2xcBatchDesc bd)
{
#define FLB_IN (U8 ? reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(d.in) + (long long)img * bd.in_bs) : d.in + (long long)img * bd.in_bs)
#define FLB_OUT (d.out + (long long)img * bd.out_bs)
#include "w2xc_first_body.inc"
#undef FLB_OUT
#undef FLB_IN
}

// (U8: d.out is the BYTES of image 0 and bd.out_bs the image stride in bytes)
template <int CIN, int COUT, bool U8>
__global__ void __launch_bounds__(256) conv3x3_last_batch(W2xcConvDesc d, int tiles_x, int ntiles, W2xcBatchDesc bd)
{
#define FLB_IN (d.in + (long long)img * bd.in_bs)
#define FLB_OUT (U8 ? reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(d.out) + (long long)img * bd.out_bs) : d.out + (long long)img * bd.out_bs)
#include "w2xc_last_body.inc"
#undef FLB_OUT
#undef FLB_IN
}

#undef FLB_SEL
#undef FLB_ONLY

template <int TPW, typename KernelT>
static hipError_t launch_tiles_batch(KernelT kernel, const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    const int tiles_x = (d.out_w + 31) / 32, tiles_y = (d.out_h + 7) / 8;
    const long long ntiles = (long long)tiles_x * tiles_y;
    if (ntiles * b.batch >= (1ll << 31) - TPW) return hipErrorInvalidValue;
    b.items = (int)ntiles;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((ntiles * b.batch + TPW - 1) / TPW)), dim3(256), 0, stream, d, tiles_x, (int)ntiles, b);
    return hipGetLastError();
}

template <bool U8>
static hipError_t launch_first_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.cin != 3) return hipErrorInvalidValue;
    if (U8 && !((d.in_ps == 3 && d.in_cs == 1) || (d.in_ps == 4 && d.in_cs == 0))) return hipErrorInvalidValue;   // (4, 0: the alpha byte of RGBA pixels, as w2xc_launch_conv)
    if (d.out_ps == 1) {   // planar out: whole pixel quads, every image's planes as aligned as image 0's
        if (((d.out_rs | d.out_cs | b.out_bs) & 3) != 0 || d.out_rs < ((d.out_w + 3) & ~3) || (((size_t)d.out) & 15) != 0) return hipErrorInvalidValue;
        switch (d.cout) {
        case 32: return launch_tiles_batch<FIRST_TPW>(conv3x3_first_batch<3, 1, true, U8>, d, b, stream);
        case 64: return launch_tiles_batch<FIRST_TPW>(conv3x3_first_batch<3, 2, true, U8>, d, b, stream);
        case 128: return launch_tiles_batch<FIRST_TPW>(conv3x3_first_batch<3, 4, true, U8>, d, b, stream);
        default: return hipErrorInvalidValue;
        }
    }
    if (d.out_ps != d.cout || d.out_cs != 1 || (b.out_bs & 3) != 0) return hipErrorInvalidValue;
    switch (d.cout) {
    case 32: return launch_tiles_batch<FIRST_TPW>(conv3x3_first_batch<3, 1, false, U8>, d, b, stream);
    case 64: return launch_tiles_batch<FIRST_TPW>(conv3x3_first_batch<3, 2, false, U8>, d, b, stream);
    case 128: return launch_tiles_batch<FIRST_TPW>(conv3x3_first_batch<3, 4, false, U8>, d, b, stream);
    default: return hipErrorInvalidValue;
    }
}

template <bool U8>
static hipError_t launch_last_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.in_ps != d.cin || d.in_cs != 1 || d.cout != 3 || (b.in_bs & 3) != 0) return hipErrorInvalidValue;   // (16-byte loads of NHWC pixels)
    if (U8 && (d.out_ps != 3 || d.out_cs != 1)) return hipErrorInvalidValue;
    switch (d.cin) {
    case 32: return launch_tiles_batch<LAST_TPW>(conv3x3_last_batch<32, 3, U8>, d, b, stream);
    case 64: return launch_tiles_batch<LAST_TPW>(conv3x3_last_batch<64, 3, U8>, d, b, stream);
    case 128: return launch_tiles_batch<LAST_TPW>(conv3x3_last_batch<128, 3, U8>, d, b, stream);
    default: return hipErrorInvalidValue;
    }
}

// d = the single-image descriptor of w2xc_launch_conv(kind, d) (its checks apply unchanged), b.in_bs / b.out_bs = image strides: floats, or -- the uint8
// side of W2XC_K_FIRST_U8 / W2XC_K_LAST_U8 -- bytes
hipError_t w2xc_launch_conv_batch(W2xcKernelKind kind, const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0 || b.batch == 0) return hipSuccess;
    if (b.batch < 0 || b.in_bs < 0 || b.out_bs < 0) return hipErrorInvalidValue;
    switch (kind) {
    case W2XC_K_FIRST: return launch_first_batch<false>(d, b, stream);
    case W2XC_K_FIRST_U8: return launch_first_batch<true>(d, b, stream);
    case W2XC_K_LAST: return d.in_shift ? hipErrorInvalidValue : launch_last_batch<false>(d, b, stream);
    case W2XC_K_LAST_U8: return d.in_shift ? hipErrorInvalidValue : launch_last_batch<true>(d, b, stream);
    default: return hipErrorInvalidValue;
    }
}
