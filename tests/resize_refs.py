"""The reference of the input-resize tests (spi_model_set_input_resize): ATen's antialiased bilinear
interpolation in float64 on the CPU, the centre crop at torchvision's offsets, and the bound the fp32
results are held to.  Nothing here goes through the project's library."""
import numpy as np
import torch

MEAN = np.float32([0.485, 0.456, 0.406])
STD = np.float32([0.229, 0.224, 0.225])
SCALE = np.float32(1) / (np.float32(255) * STD)  # the ImageNet transform: three distinct shifts
SHIFT = -MEAN / STD
UNIT_SCALE = np.float32([1, 1, 1]) / np.float32(255)
ZERO = np.float32([0, 0, 0])

# (H, W, resize_short R, crop S): a non-integer downscale; portrait (the long side's truncation); an upscale;
# 12 taps; one-pixel sources; d = RW - S = 3 (the crop offset rounds up to 2) and d = 1 (rounds down to 0)
SHAPES = [(37, 53, 24, 16), (53, 37, 24, 16), (20, 30, 36, 32), (257, 200, 36, 32), (1, 5, 8, 8), (5, 1, 8, 8),
          (33, 47, 32, 29), (16, 17, 16, 15)]


# beyond the issue's list: the kernel keeps a workgroup's weights in LDS up to 16 taps per output index
# (resample.hip: kWCap, decided from ceil(2 max(n_in, n_out) / n_out)) and above that every thread computes its
# own -- a downscale of exactly 8 (16 taps, the table full), of 8.5 (17, the first size on the other path) and
# of 15 (30 / 31 taps)
SHAPES_MANY_TAPS = [(128, 128, 16, 16), (136, 136, 16, 16), (400, 300, 20, 16)]


def pixels(seed, b, h, w, nhwc):
    shape = (b, h, w, 3) if nhwc else (b, 3, h, w)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def geometry(h, w, r, s):
    """(RH, RW, top, left): torchvision Resize(int) then CenterCrop (int(round((RH - S) / 2.0)), half to even)."""
    rh, rw = (r, r * w // h) if h <= w else (r * h // w, r)
    return rh, rw, int(round((rh - s) / 2.0)), int(round((rw - s) / 2.0))


def reference64(x_u8, nhwc, r, s):
    """float64 [B][3][S][S] in pixel units: the resample on the whole image, then the crop."""
    x = torch.from_numpy(np.ascontiguousarray(x_u8.transpose(0, 3, 1, 2)) if nhwc else x_u8)
    rh, rw, top, left = geometry(x.shape[2], x.shape[3], r, s)
    y = torch.nn.functional.interpolate(x.double(), size=(rh, rw), mode="bilinear", antialias=True, align_corners=False)
    return y[:, :, top:top + s, left:left + s].contiguous().numpy()


def reference_image(x_u8, nhwc, r, s, scale=None, shift=None):
    """The fp32 image a CPU worker feeds the module: reference64 cast to float32, then x * scale + shift
    in float32 (two roundings)."""
    y = reference64(x_u8, nhwc, r, s).astype(np.float32)
    if scale is None:
        return y
    return y * np.float32(scale).reshape(1, 3, 1, 1) + np.float32(shift).reshape(1, 3, 1, 1)


def max_taps(n_in, n_out, first, count):
    """The largest tap count of output indices first .. first + count - 1 on one axis (the integer form of
    ATen's support: centre n_in (2 i + 1) / (2 n_out), half-width max(n_in, n_out) / n_out)."""
    m = max(n_in, n_out)
    k = 0
    for i in range(first, first + count):
        c2 = n_in * (2 * i + 1)
        lo = max(0, (c2 - 2 * m + n_out) // (2 * n_out))
        hi = min(n_in, (c2 + 2 * m + n_out) // (2 * n_out))
        k = max(k, hi - lo)
    return k


def bound(h, w, r, s):
    """255 (Kx + Ky + 4) 2^-24 pixel levels: two fp32 dot products of Kx and Ky terms over values <= 255,
    one rounding per term, with weights good to about 2 ulp each."""
    rh, rw, top, left = geometry(h, w, r, s)
    return 255.0 * (max_taps(w, rw, left, s) + max_taps(h, rh, top, s) + 4) * 2.0 ** -24
