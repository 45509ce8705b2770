"""CPU: real3dportrait_amd/sr_activation.py, the one place that knows what an SR activation is (a tensor + `_r3d_fmt`, `_r3d_for`, `_r3d_bound`,
`_r3d_depth`).  Plain python over shapes and attributes: CPU tensors are enough."""
import pytest
import torch

from real3dportrait_amd import sr_activation as sa

PROTOCOL = ("_r3d_fmt", "_r3d_for", "_r3d_bound", "_r3d_depth")


def tags(t):
    return {k: getattr(t, k) for k in PROTOCOL if hasattr(t, k)}


class Consumer:
    """What a producer asks of the module it scales a SPLIT output for."""

    def __init__(self, mx):
        self.mx, self.scale = mx, torch.ones(4)

    def wants_mx(self):
        return self.mx

    def in_scale(self):
        return self.scale, 7


def test_format_table_is_the_abi():
    from real3dportrait_amd.superresolution import SynthesisBlock
    assert sa.FMT == {"none": -1, "nchw": 0, "cb8": 1, "split": 2, "split_mx": 3}
    assert SynthesisBlock._FMT is sa.FMT


@pytest.mark.parametrize("fmt,shape,dtype", [("nchw", (2, 16, 3, 5), torch.float32), ("cb8", (2, 2, 3, 5, 8), torch.float32),
                                             ("split", (2, 2, 2, 3, 5, 8), torch.float16), ("split_mx", (2, 2, 2, 3, 5, 8), torch.float16)])
def test_empty_and_logical_shape_round_trip(fmt, shape, dtype):
    y = sa.empty(fmt, 2, 16, 3, 5, "cpu")
    assert tuple(y.shape) == shape and y.dtype == dtype and y.is_contiguous()
    assert sa.fmt_of(y) == fmt and tuple(sa.logical_shape(y)) == (2, 16, 3, 5)
    assert tags(y) == ({} if fmt == "nchw" else {"_r3d_fmt": fmt})          # 'nchw' is the untagged tensor


def test_as_input_checks_the_consumer_of_a_split_tensor():
    me, other = Consumer(False), Consumer(False)
    for fmt in ("split", "split_mx"):
        x = sa.tag_split(sa.empty(fmt, 1, 16, 2, 2, "cpu"), fmt, me)
        y, f, folded = sa.as_input(x, me)
        assert y is x and f == fmt and folded is True
        with pytest.raises(RuntimeError, match="SPLIT activation was scaled for a different consumer"):
            sa.as_input(x, other)
        del x._r3d_for
        with pytest.raises(RuntimeError, match="SPLIT activation was scaled for a different consumer"):
            sa.as_input(x, me)


def test_as_input_keeps_the_tags_of_an_fp32_tensor_across_the_detach():
    bound = torch.tensor([3.0, 4.0])
    x = sa.tag_bound(sa.empty("cb8", 2, 16, 3, 5, "cpu").zero_().requires_grad_(), bound, 2)
    y, f, folded = sa.as_input(x, Consumer(False))
    assert y is not x and not y.requires_grad and f == "cb8" and folded is False
    assert tags(y) == {"_r3d_fmt": "cb8", "_r3d_bound": bound, "_r3d_depth": 2} and y._r3d_bound is bound
    z, f, folded = sa.as_input(torch.zeros(1, 3, 2, 2, dtype=torch.float64), None)          # untagged: nothing appears
    assert z.dtype == torch.float32 and f == "nchw" and folded is False and tags(z) == {}
    assert sa._keep_tags(y)._r3d_depth == 2 and sa.bound_of(y, None, layers=2) == (bound, 2)
    meter = lambda t: "measured"                                                             # noqa: E731
    assert sa.bound_of(y, meter, layers=3) == ("measured", 0)                                # 2 + 3 - 1 > MAX_DEPTH: not trusted
    assert sa.bound_of(z, meter) == ("measured", 0)


def test_out_target_downgrades_split_mx_exactly_when_one_side_has_no_records():
    for producer_mx in (False, True):
        for consumer_mx in (False, True):
            nxt = Consumer(consumer_mx)
            fmt, scale, stride = sa.out_target("split_mx", producer_mx, nxt)
            assert fmt == ("split_mx" if producer_mx and consumer_mx else "split") and scale is nxt.scale and stride == 7
            assert sa.out_target("split", producer_mx, nxt) == ("split", nxt.scale, 7)      # never upgraded
    for fmt in ("none", "nchw", "cb8"):
        assert sa.out_target(fmt, True, None) == (fmt, None, 0)
        assert sa.out_target(fmt, True, Consumer(True)) == (fmt, None, 0)                   # the fp32 formats are not scaled for anybody


@pytest.mark.parametrize("fmt", ["split", "split_mx"])
def test_out_target_needs_the_consumer_of_a_split_output(fmt):
    with pytest.raises(RuntimeError, match="needs the consumer"):
        sa.out_target(fmt, True, None)


def test_tag_functions_set_exactly_the_protocol_attributes():
    me, bound = Consumer(True), torch.tensor([1.0])
    y = torch.zeros(1, 2, 2, 2, 2, 8, dtype=torch.float16)
    assert sa.tag_split(y, "split_mx", me) is y and tags(y) == {"_r3d_fmt": "split_mx", "_r3d_for": me}
    z = torch.zeros(1, 16, 2, 2)
    assert sa.tag_bound(z, bound, 1) is z and tags(z) == {"_r3d_bound": bound, "_r3d_depth": 1}
    assert sa._tag is sa.tag_bound


def test_the_helpers_stay_importable_from_superresolution():
    from real3dportrait_amd import superresolution as sr
    assert sr._tag is sa.tag_bound and sr._keep_tags is sa._keep_tags and sr.bound_of is sa.bound_of and sr.MAX_DEPTH == sa.MAX_DEPTH
    assert callable(sr._fold_single)
    for cls in (sr.SynthesisBlock, sr.SynthesisBlockNoUp, sr.Conv2d, sr.ConvStack):         # ordinary methods of the class bodies
        assert "num_layers" in vars(cls if cls is not sr.SynthesisBlockNoUp else sr.SynthesisBlock) and callable(cls.fold_for_input)
