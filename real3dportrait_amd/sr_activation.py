"""What an SR activation is: a torch tensor plus up to four python attributes, and the one place that knows the formats.

  _r3d_fmt    absent ('nchw': fp32 [N, C, H, W]) | 'cb8' (fp32 channel-blocked [N, C/8, H, W, 8]) | 'split' | 'split_mx' (fp16 hi / lo planes
              [N, 2, C/8, H, W, 8] stored times the consumer's folded in-multiplier; split_mx: fp8 records in the lo plane for an f16mx consumer)
  _r3d_for    on a SPLIT tensor: the module whose in-multiplier it was scaled by -- only that module may consume it
  _r3d_bound  on an fp32 tensor: device float [N], a guaranteed bound on max|x| per sample
  _r3d_depth  conv layers between the last measurement and that bound

The attribute names are the protocol: bench.py, frames.py, triplane.py, scripts/ and the tests set and read them directly.  Everything here is plain
python over shapes and attributes; the only torch calls are the allocation in `empty` and the detach / contiguous of an input."""
import torch

FMT = {"none": -1, "nchw": 0, "cb8": 1, "split": 2, "split_mx": 3}      # name -> R3D_FMT_* (include/r3d_hip.h)
SPLIT_FORMATS = ("split", "split_mx")
MAX_DEPTH = 3      # a stored fp16 operand may be at most this many conv layers away from a measured / known max|x|


def fmt_of(x):
    return getattr(x, "_r3d_fmt", "nchw")


def logical_shape(x):
    """(N, C, H, W) of an activation in any format."""
    s, fmt = x.shape, fmt_of(x)
    if fmt == "nchw":
        return s
    if fmt == "cb8":
        return s[0], s[1] * 8, s[2], s[3]
    return s[0], s[2] * 8, s[3], s[4]


def empty(fmt, N, C, H, W, device):
    """An uninitialised activation [N, C, H, W] in `fmt`, tagged with it."""
    if fmt in SPLIT_FORMATS:
        y = torch.empty(N, 2, C // 8, H, W, 8, device=device, dtype=torch.float16)
    elif fmt == "cb8":
        y = torch.empty(N, C // 8, H, W, 8, device=device, dtype=torch.float32)
    else:
        return torch.empty(N, C, H, W, device=device, dtype=torch.float32)
    y._r3d_fmt = fmt
    return y


def tag_bound(y, bound, depth):
    y._r3d_bound, y._r3d_depth = bound, depth
    return y


_tag = tag_bound


def tag_split(y, fmt, consumer):
    y._r3d_fmt, y._r3d_for = fmt, consumer
    return y


def _keep_tags(x):
    """detach().to(float32).contiguous() drops python attributes: carry the range tags and the format over."""
    y = x.detach().to(torch.float32).contiguous()
    if y is not x:
        b = getattr(x, "_r3d_bound", None)
        if b is not None:
            tag_bound(y, b, int(getattr(x, "_r3d_depth", 0)))
        fmt = getattr(x, "_r3d_fmt", None)
        if fmt is not None:
            y._r3d_fmt = fmt
    return y


def bound_of(x, meter, layers=1):
    """(bound, depth) of an fp32 activation that is about to enter a chain of `layers` conv layers folded together.  The propagated
    bound loosens ~5 binades per layer and the fp16 window has ~16, so a tag (`_r3d_bound`, `_r3d_depth` = layers since the last
    measurement) is only trusted while the deepest operand of the chain stays within MAX_DEPTH layers of a measurement; otherwise
    max|x| is measured on the device (depth 0)."""
    b = getattr(x, "_r3d_bound", None)
    d = int(getattr(x, "_r3d_depth", 0))
    if b is not None and d + layers - 1 <= MAX_DEPTH:
        return b, d
    return meter(x), 0


def as_input(x, consumer):
    """(x, fmt, already_folded) for `consumer`: a SPLIT tensor must have been scaled for it (its fold is then in place); an fp32 one is
    detached with its tags kept."""
    fmt = fmt_of(x)
    if fmt in SPLIT_FORMATS:
        if getattr(x, "_r3d_for", None) is not consumer:
            raise RuntimeError("SPLIT activation was scaled for a different consumer")
        return x.contiguous(), fmt, True
    return _keep_tags(x), fmt, False


def out_target(fmt, producer_writes_mx, _next):
    """(fmt, next_scale, next_stride) of a producer's output: the SPLIT formats are scaled for `_next`, the consumer (already folded), and fp8
    records are written only by a producer that can (an f16mx block, a plain conv) for a consumer that reads them (`_next.wants_mx()`)."""
    if fmt not in SPLIT_FORMATS:
        return fmt, None, 0
    if _next is None:
        raise RuntimeError("out_format=%r needs the consumer (`_next`: its folded in-multiplier)" % fmt)
    if fmt == "split_mx" and not (producer_writes_mx and _next.wants_mx()):
        fmt = "split"
    return (fmt,) + _next.in_scale()
