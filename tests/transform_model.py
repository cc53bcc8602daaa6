"""NumPy statement of the device image transformer's arithmetic (include/dsopp_hip.h, dsopp_hip_transformer_create): CameraResizer =
cv::resize of an 8-bit single-channel image, INTER_LINEAR in its 11-bit fixed point or INTER_NEAREST, then ImageCropper = the top-left
multiple of 2^levels, and what both do to a pinhole calibration.  All in integers once the weights exist, so the device is held to it
bit for bit.  Written from the description of cv::resize, not from the kernel; pinned by tests/test_transform.py."""
import numpy as np

COEF_ONE = 2048   # INTER_RESIZE_COEF_SCALE = 1 << 11


def resized_size(n_in, ratio):
    """CameraResizer: static_cast<int>(static_cast<double>(n) * ratio) (camera_resizer.cpp:9-10)"""
    return int(float(n_in) * float(ratio))


def cropped_size(n, levels):
    """cropSizePowerOf2 (camera_image_crop.hpp:16-20)"""
    return (int(n) >> levels) << levels


def sizes(in_size, ratio, levels):
    """(width, height) -> (resized (width, height), output (width, height))"""
    resized = tuple(resized_size(n, ratio) for n in in_size)
    return resized, tuple(cropped_size(n, levels) for n in resized)


def _scale(n_in, n_out):
    return 1.0 / (float(n_out) / float(n_in))


def linear_axis(n_in, n_out):
    """first tap, second tap (clamped into the axis: its weight is 0 wherever the clamp moves it), and the two 11-bit weights of
    every output index of an axis resized from n_in to n_out pixels"""
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * _scale(n_in, n_out) - 0.5).astype(np.float32)
    whole = np.floor(f)
    s = whole.astype(np.int64)
    f = f - whole                                   # float32 - float32: stays float32
    low, high = s < 0, s >= n_in - 1
    s = np.where(low, 0, np.where(high, n_in - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    w1 = np.rint(f * np.float32(2048.0)).astype(np.int64)                       # np.rint rounds half to even
    w0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int64)
    return s, np.minimum(s + 1, n_in - 1), w0, w1


def nearest_axis(n_in, n_out):
    d = np.arange(n_out, dtype=np.float64)
    return np.minimum(np.floor(d * _scale(n_in, n_out)).astype(np.int64), n_in - 1)


def _check(src):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and min(src.shape) >= 1
    return src


def resize_linear(src, out_size):
    """cv::resize(src, Size(out_size), 0, 0, INTER_LINEAR) of H x W uint8; out_size = (width, height)"""
    src = _check(src)
    H, W = src.shape
    x0, x1, a0, a1 = linear_axis(W, out_size[0])
    y0, y1, b0, b1 = linear_axis(H, out_size[1])
    p = src.astype(np.int64)
    rows = a0[None, :] * p[:, x0] + a1[None, :] * p[:, x1]          # the horizontal pass of every source row
    out = (((b0[:, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_nearest(src, out_size):
    """cv::resize(src, Size(out_size), 0, 0, INTER_NEAREST)"""
    src = _check(src)
    H, W = src.shape
    return src[nearest_axis(H, out_size[1])[:, None], nearest_axis(W, out_size[0])[None, :]]


def crop(image, levels):
    """ImageCropper::transformImage (image_cropper.cpp:7-14)"""
    h, w = image.shape
    return image[:cropped_size(h, levels), :cropped_size(w, levels)]


def transform_image(src, ratio, levels):
    """runImageTransformers of a resizer at `ratio` and a cropper of `levels`"""
    src = _check(src)
    resized, _ = sizes((src.shape[1], src.shape[0]), ratio, levels)
    return np.ascontiguousarray(crop(resize_linear(src, resized), levels))


def transform_mask(src, ratio, levels):
    """runMaskTransformers of the same two"""
    src = _check(src)
    resized, _ = sizes((src.shape[1], src.shape[0]), ratio, levels)
    return np.ascontiguousarray(crop(resize_nearest(src, resized), levels))


def transform_calibration(in_size, intrinsics, ratio, levels):
    """CameraCalibration::resize then ::crop of a pinhole calibration (camera_calibration.cpp:33-46): -> (image_size, intrinsics)"""
    size = np.asarray(in_size, dtype=np.float64) * float(ratio)
    k = np.asarray(intrinsics, dtype=np.float64) * float(ratio)
    return np.array([float((int(v) >> levels) << levels) for v in size]), k
