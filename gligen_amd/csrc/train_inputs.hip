// The input stage of a training iteration (include/gligen_amd_train_inputs.h; reference trainer.py:329-364): q_sample, the inpainting
// mask from the boxes, z * mask and the concatenation, written as the pixel rows unet_train_step reads. One launch, one lane per
// (sample, pixel): the reads run along the pixels of one NCHW plane (coalesced), a lane's 2C + 1 (or C) outputs are contiguous.
// B H W lanes of a few loads each: a latency-class kernel whose point is one launch and no permute copies.
#include "train.h"

namespace gl {

namespace {

__global__ void train_step_inputs_kernel(const float* __restrict__ z, const float* __restrict__ noise, const int64_t* __restrict__ timesteps,
                                         const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac, int n_t,
                                         const float* __restrict__ boxes, int n_boxes, const float* __restrict__ mask_in, int inpaint, int B, int C,
                                         int H, int W, float* __restrict__ x_rows, float* __restrict__ target_rows, float* __restrict__ t_float) {
    const int HW = H * W;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // (b, pixel)
    if (i >= B * HW) return;
    const int b = i / HW, p = i - b * HW;
    const int64_t t64 = timesteps[b];
    if (p == 0) t_float[b] = (float)t64;
    const int t = (int)(t64 < 0 ? 0 : t64 >= n_t ? n_t - 1 : t64);
    const float a = sqrt_ac[t], s = sqrt_1mac[t];
    float m = 1.f;
    if (inpaint) {
        if (mask_in) {
            m = mask_in[i];
        } else {
            const int y = p / W, x = p - y * W;
            const float* bx = boxes + (size_t)b * n_boxes * 4;
            for (int k = 0; k < n_boxes; ++k) {     // int(box * size): an fp32 product, truncated towards zero
                const int x0 = (int)(bx[4 * k] * (float)W), y0 = (int)(bx[4 * k + 1] * (float)H);
                const int x1 = (int)(bx[4 * k + 2] * (float)W), y1 = (int)(bx[4 * k + 3] * (float)H);
                if (x >= x0 && x < x1 && y >= y0 && y < y1) m = 0.f;
            }
        }
    }
    const int Co = inpaint ? 2 * C + 1 : C;
    const float* zp = z + (size_t)b * C * HW + p;
    const float* np = noise + (size_t)b * C * HW + p;
    float* xo = x_rows + (size_t)i * Co;
    float* to = target_rows + (size_t)i * C;
    for (int c = 0; c < C; ++c) {
        const float zv = zp[(size_t)c * HW], nv = np[(size_t)c * HW];
        // two rounded products and one rounded sum, as torch computes a[t] * z + s[t] * noise: no contraction into an FMA
        xo[c] = __fadd_rn(__fmul_rn(a, zv), __fmul_rn(s, nv));
        to[c] = nv;
        if (inpaint) xo[C + c] = zv * m;
    }
    if (inpaint) xo[2 * C] = m;
}

}  // namespace

int train_step_inputs_launch(const TrainStepInputs& a, hipStream_t s) {
    if (a.B < 1 || a.C < 1 || a.H < 1 || a.W < 1 || a.n_t < 1 || a.n_boxes < 0)
        return set_error(GL_ERR_ARG, "train_step_inputs: B, C, H, W and n_t must be positive, n_boxes >= 0");
    if ((int64_t)a.B * a.H * a.W * (2 * (int64_t)a.C + 1) >= (int64_t(1) << 31))
        return set_error(GL_ERR_ARG, "train_step_inputs: B H W (2 C + 1) must stay below 2^31");
    if (!a.z || !a.noise || !a.timesteps || !a.sqrt_ac || !a.sqrt_1mac || !a.x_rows || !a.target_rows || !a.t_float)
        return set_error(GL_ERR_ARG, "train_step_inputs: null pointer");
    if (a.inpaint) {
        if ((a.boxes != nullptr) == (a.mask != nullptr))
            return set_error(GL_ERR_ARG, "train_step_inputs: an inpainting step takes the boxes or an explicit mask, exactly one of them");
        if (a.boxes && a.H != a.W)
            return set_error(GL_ERR_ARG, "train_step_inputs: the mask drawn from boxes is square (inpaint_mask_func.py:22); H = %d, W = %d", a.H, a.W);
        if (a.boxes && a.n_boxes < 1) return set_error(GL_ERR_ARG, "train_step_inputs: boxes given, n_boxes = 0");
    } else if (a.boxes || a.mask) {
        return set_error(GL_ERR_ARG, "train_step_inputs: boxes / mask are the inpainting model's inputs (inpaint = 0)");
    }
    const int n = a.B * a.H * a.W;
    hipLaunchKernelGGL(train_step_inputs_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, a.z, a.noise, a.timesteps, a.sqrt_ac, a.sqrt_1mac, a.n_t, a.boxes,
                       a.n_boxes, a.mask, a.inpaint, a.B, a.C, a.H, a.W, a.x_rows, a.target_rows, a.t_float);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl
