"""-m gpu: cj_reduce_kernel / cj_apply_kernel (csrc/colour_jitter.hip) through findtextcenternet_amd.ColorJitter.apply and the C ABI of
include/ftc_colour_jitter.h, BIT FOR BIT against the NumPy oracle of tests/colour_jitter_operands.py.

  fixtures     all 24 orders and all 16 masks at 3 x 5 x 7, the four shapes (one pixel; W and H * W no multiple of 4; two workgroups per image on the
               scalar and on the 16-byte path), the ends of ColorJitter(0.5, 0.5, 0.5, 0.5)'s ranges, the hand-made pixel table with its hue factors
  independence image b of a B = 3 call equals its B = 1 call; in place equals out of place; a base pointer 4 bytes off a 16-byte boundary (the scalar
               path) equals the aligned call (the 16-byte path where H * W allows it)
  guards       `out` lies inside a larger buffer of NaN sentinels, which no call may touch; a refused call writes nothing

tests/test_colour_jitter_operands_host.py proves on the CPU what the fixtures reach and that their float64 gray sums are exact in any order, so the
contrast mean has one value whatever the partition.  One further test compares with torchvision itself where it is installed."""
import ctypes as C

import numpy as np
import pytest
import torch

import colour_jitter_operands as O
import step_operands as S
from findtextcenternet_amd import ColorJitter, JitterParams
from findtextcenternet_amd import _lib as L

pytestmark = pytest.mark.gpu
_FIXTURES = O.all_fixtures()
SENTINEL = 0x7fc0beef
PAD = 64                                   # sentinel words in front of and behind `out` (256 bytes: the 16-byte alignment of the middle is kept)


def _guarded(shape, shift: int = 0):
    """-> (whole buffer, the view of `shape` inside it, PAD + shift words in).  shift = 1 puts the view 4 bytes off a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD + shift,), SENTINEL, dtype=torch.int32, device="cuda")
    view = buf[PAD + shift:PAD + shift + n].view(torch.float32).view(*shape)
    assert view.data_ptr() % 16 == 4 * shift
    return buf, view


def _intact(buf, shape, shift: int = 0) -> bool:
    n = int(np.prod(shape))
    host = buf.cpu().numpy()
    return bool((host[:PAD + shift] == SENTINEL).all() and (host[PAD + shift + n:] == SENTINEL).all())


def _apply(imgs: np.ndarray, ps, shift: int = 0, inplace: bool = False) -> np.ndarray:
    buf_in, x = _guarded(imgs.shape, shift)
    x.copy_(torch.from_numpy(imgs))
    if inplace:
        got = ColorJitter.apply(x, ps, out=x)
        assert got is x
        buf_out = buf_in
    else:
        buf_out, out = _guarded(imgs.shape, shift)
        got = ColorJitter.apply(x, ps, out=out)
        assert got is out
    torch.cuda.synchronize()
    assert _intact(buf_out, imgs.shape, shift) and _intact(buf_in, imgs.shape, shift), "words in front of or behind a buffer were written"
    if not inplace:
        S.assert_bytes(x.cpu().numpy(), imgs, "the input of an out-of-place call was written")
    return got.cpu().numpy()


@pytest.fixture(scope="module")
def want():
    return {name: O.jitter_batch(imgs, ps) for name, (imgs, ps) in _FIXTURES.items()}


@pytest.mark.parametrize("name", list(_FIXTURES))
def test_fixture_bitwise(name, want):
    imgs, ps = _FIXTURES[name]
    S.assert_bits(_apply(imgs, ps), want[name], name)


@pytest.mark.parametrize("hw", O.SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_batch_slot_path_and_aliasing_do_not_matter(hw, want):
    name = f"shape_{hw[0]}x{hw[1]}"
    imgs, ps = _FIXTURES[name]
    for b in range(3):                                               # image b alone, as [1, 3, H, W] and as [3, H, W]
        S.assert_bits(_apply(imgs[b:b + 1], ps[b:b + 1])[0], want[name][b], (name, b, "B = 1"))
    S.assert_bits(_apply(imgs[1], ps[1]), want[name][1], (name, "three dimensions"))
    S.assert_bits(_apply(imgs, ps, inplace=True), want[name], (name, "in place"))
    S.assert_bits(_apply(imgs, ps, shift=1), want[name], (name, "base 4 bytes off"))
    S.assert_bits(_apply(imgs, ps, shift=1, inplace=True), want[name], (name, "base 4 bytes off, in place"))
    S.assert_bits(_apply(imgs[::-1].copy(), ps[::-1])[::-1], want[name], (name, "slots reversed"))


def test_forward_draws_once_for_the_batch_and_returns_a_new_tensor():
    imgs = np.stack([O.image(33, 130, 900 + i) for i in range(2)])
    x = torch.from_numpy(imgs).cuda()
    jit = ColorJitter(0.5, 0.5, 0.5, 0.5)
    torch.manual_seed(11)
    y = jit(x)
    after = torch.rand(1)
    torch.manual_seed(11)
    p = jit.draw()
    assert torch.equal(after, torch.rand(1))                         # one draw: the generator stands where a single get_params leaves it
    assert y is not x and y.data_ptr() != x.data_ptr() and y.shape == x.shape
    S.assert_bytes(x.cpu().numpy(), imgs, "forward wrote its input")
    S.assert_bits(y.cpu().numpy(), O.jitter_batch(imgs, [p, p]), "forward")
    torch.manual_seed(11)
    S.assert_bits(jit.forward(x[0]).cpu().numpy(), O.jitter_image(imgs[0], p), "forward on [3, H, W]")
    S.assert_bits(ColorJitter()(x).cpu().numpy(), imgs, "the default transform is the identity")


def test_refusals_write_nothing():
    imgs, ps = _FIXTURES["shape_5x7"]
    buf, out = _guarded(imgs.shape)
    x = torch.from_numpy(imgs).cuda()
    p = JitterParams((0, 1, 2, 3), 1.2, 0.8)
    for bad_img, exc in ((x.to(torch.uint8), TypeError), (x.cpu(), RuntimeError), (x.half(), RuntimeError), (x[:, :2], ValueError), (x[..., ::2], ValueError)):
        with pytest.raises(exc):
            ColorJitter.apply(bad_img, [p] * 3, out=None)
    with pytest.raises(ValueError, match="JitterParams for 3"):
        ColorJitter.apply(x, [p] * 2, out=out)
    with pytest.raises(ValueError, match="out must be"):
        ColorJitter.apply(x, [p] * 3, out=out[:2])
    for bad in (JitterParams((0, 1, 1, 3), 1.2), JitterParams((0, 1, 2, 3), hue=0.7), JitterParams((0, 1, 2, 3), saturation=-1.0)):
        with pytest.raises(ValueError):
            ColorJitter.apply(x, [p, bad, p], out=out)
    # and through the C ABI, with real device pointers: every refusal comes before the first launch
    lib = L.load()
    arr = (L.CjDesc * 3)()
    for d in arr:
        d.order[:] = (0, 1, 2, 3)
        d.factor[:] = (1.2, 0.8, 1.0, 0.0)
        d.mask = 3
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    ws = torch.zeros(3, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda d=arr, B=3, H=5, W=7, w=ws.data_ptr(), wb=24: lib.ftc_colour_jitter(d, dev.data_ptr(), B, H, W, x.data_ptr(), out.data_ptr(), w, wb, stream)      # noqa: E731
    assert call(wb=23) == -1 and b"workspace" in lib.ftc_last_error()
    assert call(w=None, wb=0) == -1 and b"workspace" in lib.ftc_last_error()
    assert call(B=0) == -1 and call(H=0) == -1 and call(W=0) == -1
    arr[2].order[:] = (0, 0, 2, 3)
    assert call() == -1 and b"permutation" in lib.ftc_last_error()
    arr[2].order[:] = (0, 1, 2, 3)
    arr[1].factor[3] = 0.75
    assert call() == -1 and b"hue" in lib.ftc_last_error()
    arr[1].factor[3] = float("nan")
    assert call() == -1 and b"finite" in lib.ftc_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all(), "a refused call wrote"
    arr[1].factor[3] = 0.0                                           # the same call with valid records runs, and without contrast it needs no workspace
    L.check(call(), "ftc_colour_jitter")
    for d in arr:
        d.mask = 1
    dev1 = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()          # the device copy must be the records the host copy holds
    buf2, out2 = _guarded(imgs.shape)
    L.check(lib.ftc_colour_jitter(arr, dev1.data_ptr(), 3, 5, 7, x.data_ptr(), out2.data_ptr(), None, 0, stream), "ftc_colour_jitter")
    torch.cuda.synchronize()
    S.assert_bits(out2.cpu().numpy(), O.jitter_batch(imgs, [JitterParams((0, 1, 2, 3), brightness=O.f32(1.2))] * 3), "brightness alone, no workspace")
    S.assert_bits(out.cpu().numpy(), O.jitter_batch(imgs, [JitterParams((0, 1, 2, 3), O.f32(1.2), O.f32(0.8))] * 3), "brightness and contrast")


def test_against_torchvision_where_it_is_installed():
    """torchvision's own functional ops on the CPU with the same parameters.  Without contrast: bit for bit.  With contrast as the last step: torch's mean
    is a float32 reduction in its own order, so the mean may sit one fp32 step away, and the elements it scales with it: (1 - f) * 2^-24 from the mean
    plus one rounding of the sum, 2^-23 in all for f in [0, 2]."""
    pytest.importorskip("torchvision")
    import torchvision.transforms.functional as TF
    fns = (TF.adjust_brightness, TF.adjust_contrast, TF.adjust_saturation, TF.adjust_hue)

    def through_torchvision(img, p):
        t = torch.from_numpy(img.copy())
        for op in p.order:
            f = (p.brightness, p.contrast, p.saturation, p.hue)[op]
            if f is not None:
                t = fns[op](t, f)
        return t.numpy()

    imgs, ps = _FIXTURES["shape_33x130"]
    free = [JitterParams(p.order, p.brightness, None, p.saturation, p.hue) for p in ps] + [JitterParams((3, 0, 2, 1), O.f32(1.4), None, O.f32(0.6), O.f32(-0.4))]
    for im, p in zip(list(imgs) + [imgs[0]], free):
        S.assert_bits(_apply(im, p), through_torchvision(im, p), ("torchvision, no contrast", p))
    pimg, pps = O.pixel_fixture()
    for im, p in zip(pimg[:8], pps[:8]):
        S.assert_bits(_apply(im, p), through_torchvision(im, p), ("torchvision, pixel table", p))
    last = JitterParams((3, 0, 2, 1), O.f32(1.4), O.f32(0.7), O.f32(0.6), O.f32(-0.4))
    got, ref = _apply(imgs[0], last), through_torchvision(imgs[0], last)
    assert float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) <= 2.0 ** -23
