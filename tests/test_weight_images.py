"""CPU: the weight images of ops_unet are typed (WeightImage), and every launch wrapper refuses an image of the wrong precision, layout or
scale folding before it calls the library -- a bf16x3 image and an fp32 image have the same shape and bytes, so nothing else could tell."""
import pytest
import torch

from musicfpaugment_amd import ops_unet as K


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called")
    monkeypatch.setattr(K, "lib", refuse)


def test_weight_image_forms():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(9, 64, 64, generator=g)
    sc = torch.rand(64, generator=g) + 0.5
    row0 = K.weight_image(w, 0)
    assert row0.t is w and (row0.precision, row0.layout, row0.scale_folded) == (0, 0, False)
    assert torch.equal(K.weight_image(w, 1).t, K.split_bf16x3(w))
    assert torch.equal(K.weight_image(w, 1, 2).t, K.split_bf16x3_frag(w, 2))
    assert torch.equal(K.weight_image(w, 0, 2).t, K.frag_f32(w))
    folded = K.weight_image(w, 1, 2, scale=sc)
    assert folded.scale_folded and torch.equal(folded.t, K.split_bf16x3_frag(w * sc[None, :, None], 2))
    for prec in (0, 1):                                            # layout 1 (the 32 x 32 x 16 fragment order) exists at no precision
        with pytest.raises(ValueError):
            K.weight_image(w, prec, 1)
    with pytest.raises(ValueError):
        K.split_bf16x3_frag(w, 1)


def test_untyped_operands_are_taken_as_the_image_the_launch_reads():
    """A bare tensor or a (layout, tensor) pair carries nothing to check: it stands for the image the launch asks for."""
    t = torch.zeros(9, 64, 64)
    assert K._operand(t, "conv", 1, (0, 1, 2)) == K.WeightImage(t, 1, 0, False)
    assert K._operand((2, t), "wff", 1, (1, 2), (True,)) == K.WeightImage(t, 1, 2, True)
    assert K._operand(t, "upconv", 0, (2,), (True,)) == K.WeightImage(t, 0, 2, True)
    img = K.weight_image(t, 1, 2)
    assert K._operand(img, "conv", 1, (0, 1, 2)) is img


def test_a_mismatched_image_raises_before_any_library_call(no_library):
    g = torch.Generator().manual_seed(4)
    w = torch.randn(9, 64, 64, generator=g)
    sc, sh = torch.ones(64), torch.zeros(64)
    x = torch.randn(1, 8, 20, 64, generator=g)
    for img, prec in [(K.weight_image(w, 0), 1), (K.weight_image(w, 1), 0), (K.weight_image(w, 1, 2), 0),
                      (K.weight_image(w, 0, 2), 0)]:
        with pytest.raises(ValueError):
            K.conv3x3_fused(x, img, sc, sh, precision=prec)
    wt = torch.randn(4, 64, 64, generator=g)
    for img, prec in [(K.weight_image(wt, 1), 0), (K.weight_image(wt, 0), 1), (K.weight_image(wt, 1, 2), 1)]:
        with pytest.raises(ValueError):
            K.convT2x2(x, img, torch.zeros(64), precision=prec)
    skip, low = torch.randn(1, 8, 20, 64, generator=g), torch.randn(1, 4, 10, 128, generator=g)
    wsk, wup = K.weight_image(w, 1, 2, scale=sc), K.weight_image(torch.randn(16, 64, 128, generator=g), 1, 2)._replace(scale_folded=True)
    for a, b, prec in [(wsk, wup, 0),                                                      # bf16x3 images, fp32 launch
                       (K.weight_image(w, 0, 2, scale=sc), wup, 1),                        # one of each precision
                       (K.weight_image(w, 1, 2), wup, 1),                                  # the scale not folded in
                       (K.weight_image(w, 1, scale=sc), wup, 1)]:                          # the row image
        with pytest.raises(ValueError):
            K.upconv_fused(skip, low, a, b, sh, torch.zeros(4, 4, 64), 64, precision=prec)
