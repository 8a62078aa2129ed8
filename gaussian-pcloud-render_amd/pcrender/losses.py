"""The photometric loss of a training loop, evaluated by the library (C ABI gsr_image_loss_forward / gsr_image_loss_backward):

    frames, _ = rasterize_views(...)                    # [V,3,h*ss,w*ss], as the rasterizer returns them
    loss = photometric_loss(frames, target, 0.2, ss)    # [V]
    loss.sum().backward()                               # frames.grad is the dL_dpix of the render backward

`photometric_loss` is (1 - lambda) L1 + lambda (1 - SSIM) per view with the 11 x 11 Gaussian window (sigma 1.5, zero padding) nearly
every Gaussian-splat trainer uses.  With super_sample = 2 the frames are twice the target's size each way and the loss compares the
mean of every 2 x 2 block -- the reference caller's bilinear down-filter at that rate (raster_passes._finish) -- so a training loop
needs neither the down-filter nor a torch loss.  Other rates are refused: down-filter first and pass super_sample = 1.
`image_metrics` is the same kernel without a gradient: L1, SSIM, MSE and PSNR per view, on the device.

There is no CPU path: tensors are float32 on a HIP device.
"""
import torch
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization import _native


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target, lambda_dssim, super_sample):
        image_c, target_c = image.contiguous(), target.contiguous()
        device, V, W, H, _ = _native._loss_frames("photometric_loss", image_c, target_c, super_sample)
        state = _native.image_loss_state(V, W, H, device)
        terms = _native.image_loss_forward(image_c, target_c, lambda_dssim, super_sample, state=state)
        ctx.save_for_backward(image_c, target_c)
        ctx.state, ctx.lambda_dssim, ctx.super_sample = state, lambda_dssim, super_sample
        return terms[:, 3].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        image_c, target_c = ctx.saved_tensors
        grad = _native.image_loss_backward(image_c, target_c, ctx.lambda_dssim, ctx.super_sample, ctx.state,
                                           dL_dloss=grad_loss.to(torch.float32).contiguous())
        return grad, None, None, None


def photometric_loss(image, target, lambda_dssim=0.2, super_sample=1):
    """[V] per-view losses (1 - lambda_dssim) L1 + lambda_dssim (1 - SSIM) of the frames image [V,3,H*ss,W*ss] against target
    [V,3,H,W]; differentiable with respect to image (the target gets no gradient)."""
    return _PhotometricLoss.apply(image, target, float(lambda_dssim), int(super_sample))


def image_metrics(image, target, super_sample=1):
    """dict of [V] tensors l1, ssim, mse and psnr = -10 log10(mse) of the frames against the target; no gradient, no state block"""
    with torch.no_grad():
        terms = _native.image_loss_forward(image.detach().contiguous(), target.detach().contiguous(), 0.0, super_sample, state=None)
        mse = terms[:, 2]
        return {"l1": terms[:, 0], "ssim": terms[:, 1], "mse": mse, "psnr": -10.0 * torch.log10(mse)}
