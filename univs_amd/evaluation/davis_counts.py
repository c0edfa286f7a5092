"""The counts of a DAVIS evaluation, per video: everything J (region similarity) and F (boundary measure) need, for every pair of a
ground-truth object and a result object (davis.py).

  davis_video_counts   the HIP kernel (csrc/davis_count.hip) behind `ops._call`: GPU tensors only, None where it does not cover
  davis_counts_aten    the same five tensors from torch ops on any device: the fallback, the yardstick, the CPU path
  davis_counts         the kernel on GPU tensors where it covers the call, else the ATen formulation

gt is uint8 [T, H, W], the raw id maps of the annotation PNGs (255 = void), pred uint8 [T, H, W], the bytes of the result PNGs.  gt ids
1..G and pred ids 1..P are the objects; every other value is background.  With `use_void` the void pixels are taken out of both sides
(`mask & ~void`, the unsupervised task); without it the result stays as it is there (the semi-supervised task passes no void mask); the
gt's 255 is never an object.  All three return int32 tensors

  region [G, P, T, 2]   (intersection, union) of gt object i and result object j in frame t (metrics.py:29-30)
  n_gt [G, T]           boundary pixels of gt object i, as `_seg2bmap` marks them (metrics.py:154-165)
  n_fg [P, T]           the same for result object j
  match [G, P, T, 2]    (gt boundary pixels of i inside the boundary of j dilated by disk(radius), result boundary pixels of j inside the
                        dilated boundary of i) (metrics.py:87-93)
"""
import torch

from .. import ops
from . import _counts

MAX_OBJECTS = 32      # csrc/davis_count.hip: DV_MAX_OBJ, one bit per object
R_MAX = 36            # DV_R_MAX: the halo in LDS (the radius of a 4K frame)


def _check(name, gt, pred, G, P, radius):
    _counts.check_uint8_pair(name, gt, pred)
    if int(G) < 1 or int(P) < 1 or int(G) > 254 or int(P) > 255:
        raise RuntimeError(f"{name}: object counts G={G} P={P}")
    if int(radius) != radius or int(radius) < 1:
        raise RuntimeError(f"{name}: radius {radius}")


def _outputs(G, P, T, device):
    return (torch.zeros((G, P, T, 2), dtype=torch.int32, device=device), torch.zeros((G, T), dtype=torch.int32, device=device),
            torch.zeros((P, T), dtype=torch.int32, device=device), torch.zeros((G, P, T, 2), dtype=torch.int32, device=device))


def davis_video_counts(gt, pred, G, P, radius, use_void):
    """(region, n_gt, n_fg, match) from csrc/davis_count.hip on the tensors' device and current stream; None where the kernel does not
    cover the call (G or P > 32, radius > R_MAX, T H W >= 2^31): the caller keeps `davis_counts_aten`.  CPU tensors raise, as in every
    wrapper of ops.py."""
    name = "davis_video_counts"
    _counts.admit(name, gt, pred, _check, G, P, radius)
    T, H, W = (int(v) for v in gt.shape)
    G, P, radius = int(G), int(P), int(radius)
    if G > MAX_OBJECTS or P > MAX_OBJECTS or radius > R_MAX or T * H * W >= 2 ** 31:
        return None
    gt, pred = gt.contiguous(), pred.contiguous()
    return _counts.launch(name, "univs_davis_counts", gt, _outputs(G, P, T, gt.device), ops._ptr(gt), ops._ptr(pred), T, H, W, G, P, radius,
                          1 if use_void else 0)


def disk(radius, device=None):
    """float32 [2 r + 1, 2 r + 1]: the offsets with dx^2 + dy^2 <= r^2 (what skimage.morphology.disk documents)."""
    a = torch.arange(-radius, radius + 1, device=device)
    return ((a[:, None] ** 2 + a[None, :] ** 2) <= radius * radius).to(torch.float32)


def seg2bmap(seg):
    """`_seg2bmap` (metrics.py:154-165) on bool [..., H, W]: a pixel is boundary where it differs from its east, south or south-east
    neighbour; the last row compares east only, the last column south only, the bottom-right pixel is never boundary."""
    b = torch.zeros_like(seg)
    b[..., :-1, :-1] = (seg[..., :-1, :-1] ^ seg[..., :-1, 1:]) | (seg[..., :-1, :-1] ^ seg[..., 1:, :-1]) | (seg[..., :-1, :-1] ^ seg[..., 1:, 1:])
    b[..., -1, :-1] = seg[..., -1, :-1] ^ seg[..., -1, 1:]
    b[..., :-1, -1] = seg[..., :-1, -1] ^ seg[..., 1:, -1]
    return b


def davis_counts_aten(gt, pred, G, P, radius, use_void):
    """(region, n_gt, n_fg, match) on the tensors' device, CPU or GPU: one-hot planes per object, boundaries by shifted comparisons, the
    dilation as a zero-padded `conv2d` with the disk."""
    _check("davis_counts_aten", gt, pred, G, P, radius)
    G, P, r = int(G), int(P), int(radius)
    T, H, W = (int(v) for v in gt.shape)
    dev = gt.device
    pred = pred.to(dev)
    void = gt == 255
    g = torch.where(gt > G, torch.zeros_like(gt), gt)                # 255 is never an object
    p = torch.where(pred > P, torch.zeros_like(pred), pred)
    if use_void:
        p = torch.where(void, torch.zeros_like(p), p)
    # region: one table of (gt id, result id) cells per frame
    cells = (G + 1) * (P + 1)
    cell = g.reshape(T, -1).to(torch.int64) * (P + 1) + p.reshape(T, -1).to(torch.int64) + cells * torch.arange(T, device=dev)[:, None]
    table = torch.bincount(cell.reshape(-1), minlength=cells * T).reshape(T, G + 1, P + 1)
    inter = table[:, 1:, 1:]
    union = table[:, 1:, :].sum(dim=2)[:, :, None] + table[:, :, 1:].sum(dim=1)[:, None, :] - inter
    region = torch.stack([inter, union], dim=-1).permute(1, 2, 0, 3).to(torch.int32).contiguous()
    # boundaries and their dilations
    gm = g[None] == torch.arange(1, G + 1, device=dev, dtype=torch.uint8)[:, None, None, None]      # [G, T, H, W]
    pm = p[None] == torch.arange(1, P + 1, device=dev, dtype=torch.uint8)[:, None, None, None]
    gb, pb = seg2bmap(gm), seg2bmap(pm)
    n_gt = gb.sum(dim=(2, 3)).to(torch.int32)
    n_fg = pb.sum(dim=(2, 3)).to(torch.int32)
    k = disk(r, dev)[None, None]

    def dilate(b):                                                   # (sums of at most (2 r + 1)^2 ones: exact in float32)
        n = b.shape[0]
        return (torch.nn.functional.conv2d(b.reshape(n * T, 1, H, W).to(torch.float32), k, padding=r) > 0.5).reshape(n, T, H * W)
    acc = torch.float32 if H * W < 2 ** 24 else torch.float64        # the sums below are pixel counts of one frame
    gd, pd = dilate(gb).to(acc), dilate(pb).to(acc)
    gbf, pbf = gb.reshape(G, T, H * W).to(acc), pb.reshape(P, T, H * W).to(acc)
    m0 = torch.einsum("gtn,ptn->gpt", gbf, pd)
    m1 = torch.einsum("gtn,ptn->gpt", gd, pbf)
    match = torch.stack([m0, m1], dim=-1).round().to(torch.int32).contiguous()
    return region, n_gt, n_fg, match


def davis_counts(gt, pred, G, P, radius, use_void):
    """(region, n_gt, n_fg, match): the kernel on GPU tensors where it covers the call, else the ATen formulation."""
    return _counts.kernel_else_aten(davis_video_counts, davis_counts_aten, gt, pred, G, P, radius, use_void)
