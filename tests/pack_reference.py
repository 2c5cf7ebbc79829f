"""The three packed-filter layouts of include/amyloid_yolo.h in NumPy, built by reshape / transpose / pad from the layouts the header
documents -- no index arithmetic taken from the kernels (csrc/ay_pack.h).  tests/test_pack_cpu.py checks this file against itself,
tests/test_gpu_train_bf16_paths.py::test_pack_batch_against_single_packers checks the library's packers against it.

Images are float32 arrays in the documented axis order; `bits` rounds one to the stored 16-bit type with torch's CPU conversion (round
to nearest even) and returns the flat uint16 image."""
import numpy as np
import torch


def _pad_axis(a, axis, n):
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, n - a.shape[axis])
    return np.pad(a, pad)


def forward_image(w_oihw, cout_pad):
    """ay_pack_conv_weights_*: OIHW [cout][cin][k][k], cin a multiple of 16 -> [cin/16][k*k][2][cout_pad][8], zero rows cout..cout_pad;
    input channel = chunk * 16 + half * 8 + j"""
    w = np.asarray(w_oihw, dtype=np.float32)
    cout, cin, k, _ = w.shape
    assert cin % 16 == 0 and cout_pad >= cout
    img = w.reshape(cout, cin // 16, 2, 8, k * k).transpose(1, 4, 2, 0, 3)    # (co, chunk, half, j, tap) -> (chunk, tap, half, co, j)
    return _pad_axis(img, 3, cout_pad)


def _as_input_channels(w_iohw_like, cin_pad):
    """forward_image of a filter whose OUTPUT channels are the data gradient's: its input channels padded to whole chunks of 16"""
    w = _pad_axis(w_iohw_like, 1, (w_iohw_like.shape[1] + 15) // 16 * 16)
    return forward_image(w, cin_pad)


def dgrad_image(w_oihw, cin_pad):
    """ay_pack_dgrad_weights_bf16: the forward image of W'[ci][co][kh][kw] = W[co][ci][k-1-kh][k-1-kw] ->
    [ceil(cout/16)][k*k][2][cin_pad][8]"""
    w = np.asarray(w_oihw, dtype=np.float32)
    return _as_input_channels(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3), cin_pad)


# ay_conv_dgrad_s2_bf16's table: window row (column) 0, 1 of parity class 0, 1 holds this filter row (column), None = an empty slot
S2_TAPS = {0: (1, None), 1: (2, 0)}


def dgrad_s2_images(w_oihw, cout_pad, cin_pad):
    """ay_pack_dgrad_s2_weights_bf16 (3x3 filters): [class py*2+px][cout_pad/16][window tap oy*2+ox][2][cin_pad][8]"""
    w = np.asarray(w_oihw, dtype=np.float32)
    cout, cin = w.shape[:2]
    assert w.shape[2:] == (3, 3) and cout_pad % 16 == 0
    out = []
    for py in (0, 1):
        for px in (0, 1):
            win = np.zeros((cout, cin, 2, 2), np.float32)
            for oy, kh in enumerate(S2_TAPS[py]):
                for ox, kw in enumerate(S2_TAPS[px]):
                    if kh is not None and kw is not None:
                        win[:, :, oy, ox] = w[:, :, kh, kw]
            out.append(_as_input_channels(_pad_axis(win.transpose(1, 0, 2, 3), 1, cout_pad), cin_pad))
    return np.stack(out)


_TORCH = {"bf16": torch.bfloat16, "f16": torch.float16}


def bits(img, dtype="bf16"):
    t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(_TORCH[dtype])
    return t.view(torch.int16).numpy().view(np.uint16).reshape(-1)


def values(img_bits, dtype="bf16"):
    """the numbers a flat uint16 image holds (float32)"""
    return torch.from_numpy(np.ascontiguousarray(img_bits).view(np.int16)).view(_TORCH[dtype]).float().numpy()
