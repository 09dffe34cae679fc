// w2xc_gather_batch.hip -- conv3x3_last_gather_x4_batch: the W2XC_K_LAST_GATHER launch of the fp32 chain (w2xc_split.hip, conv3x3_last_gather_x4) for
// `batch` images of identical geometry in one launch (w2xc_convert_batch*): blockIdx.y = image, whose partial tap planes start in_bs floats and whose
// output plane starts out_bs floats after image 0's.  Per image the same sum in the same order -- taps outer, 64-plane blocks inner, bias, LeakyReLU --
// as the single-image kernel: bit-identical.
#include "w2xc_kernels.h"
#include "w2xc_device.h"

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte global access on a dword-aligned address

__global__ void __launch_bounds__(256) conv3x3_last_gather_x4_batch(const float *G, int halves, long long hs, long long ps, long long rs, const float *bias,
                                                                    float *out, long long out_rs, int out_h, int out_w, long long in_bs, long long out_bs)
{
    G += (long long)blockIdx.y * in_bs;
    out += (long long)blockIdx.y * out_bs;
    const int gw = (out_w + 3) >> 2;
    const long long total = (long long)out_h * gw;
    const float b = bias[0];
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int y = (int)(idx / gw), x = (int)(idx - (long long)y * gw) * 4;
        if (x + 4 <= out_w) {
            f32x4u v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const float *g = G + tap * ps + (long long)(y + tap / 3) * rs + (x + tap % 3);
                for (int hf = 0; hf < halves; hf++) v += *reinterpret_cast<const f32x4u *>(g + hf * hs);
            }
            f32x4u o;
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = leaky(v[e] + b);
            *reinterpret_cast<f32x4u *>(out + (long long)y * out_rs + x) = o;
        } else {
            for (int xx = x; xx < out_w; xx++) {
                float v = 0.0f;
#pragma unroll
                for (int tap = 0; tap < 9; tap++) {
                    const float *g = G + tap * ps + (long long)(y + tap / 3) * rs + (xx + tap % 3);
                    for (int hf = 0; hf < halves; hf++) v += g[hf * hs];
                }
                out[(long long)y * out_rs + xx] = leaky(v + b);
            }
        }
    }
}

// d = the single-image descriptor of the gather launch (planar partial planes in, planar output plane: the conv3x3_last_gather_x4 form), b = image strides
hipError_t w2xc_launch_last_gather_batch(const W2xcConvDesc &d, W2xcBatchDesc b, hipStream_t stream)
{
    if (d.out_w <= 0 || d.out_h <= 0 || b.batch == 0) return hipSuccess;
    if (b.batch < 0 || b.batch > 65535 || d.in_ps > 1 || d.out_ps != 1) return hipErrorInvalidValue;
    const long long groups = (long long)d.out_h * ((d.out_w + 3) >> 2);
    // (the single-image launch's grid per image, capped so that a batch still keeps every CU busy without a grid of millions of blocks)
    long long gx = (groups + 255) / 256;
    if (gx > 65536) gx = 65536;
    hipLaunchKernelGGL(conv3x3_last_gather_x4_batch, dim3((unsigned)gx, (unsigned)b.batch), dim3(256), 0, stream, d.in, d.halves, d.in_ts, d.in_gs, d.in_rs,
                       d.bias, d.out, d.out_rs, d.out_h, d.out_w, b.in_bs, b.out_bs);
    return hipGetLastError();
}
