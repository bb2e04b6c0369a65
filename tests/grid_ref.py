"""The picture of a set of modality tensors, written out from its definition (DESIGN.md "The image grid") in CPU float32 torch and
with none of the package's code: the shape rules, the channel rule and the centring source by source, the concatenation, the grid
tile by tile, and the quantisation operation by operation.  Every comparison against it is bit for bit."""
import torch


def as_images(t):
    """[n] -> [n,1,1,1], [n,a] -> [n,1,1,a], [n,a,b] -> [n,1,a,b], [n,c,h,w] as it is; more dimensions cannot be shown."""
    if t.dim() > 4:
        raise AttributeError("Can't visualize data with more than 3 dimensions")
    if t.dim() == 0:
        raise AttributeError("a batch dimension is needed")
    n = t.shape[0]
    rest = list(t.shape[1:])
    return t.reshape([n] + [1] * (3 - len(rest)) + rest)


def three_channels(x):
    """The channel rule on [n, c, h, w]: c = 1 replicated, c = 2 with a third channel of zeros, c >= 3 the first three."""
    n, c, h, w = x.shape
    out = torch.zeros(n, 3, h, w, dtype=torch.float32)
    for ch in range(3):
        if c == 1:
            out[:, ch] = x[:, 0]
        elif c == 2:
            if ch < 2:
                out[:, ch] = x[:, ch]
        else:
            out[:, ch] = x[:, ch]
    return out


def centred(x, H, W):
    """[n, 3, h, w] inside [n, 3, H, W] zeros: floor((H - h) / 2) rows above, floor((W - w) / 2) columns to the left."""
    n, _, h, w = x.shape
    out = torch.zeros(n, 3, H, W, dtype=torch.float32)
    top, left = (H - h) // 2, (W - w) // 2
    out[:, :, top:top + h, left:left + w] = x
    return out


def adapt_shape(data):
    """{name: tensor} -> ({name: [n, 3, H, W]}, (3, H, W)), H and W the largest height and width."""
    imgs = {m: three_channels(as_images(t.detach().to("cpu", torch.float32))) for m, t in data.items()}
    H = max(x.shape[2] for x in imgs.values())
    W = max(x.shape[3] for x in imgs.values())
    return {m: centred(x, H, W) for m, x in imgs.items()}, (3, H, W)


def make_grid(tiles, nrow, padding=2, pad_value=0.0):
    """[T, 3, H, W] -> [3, Hg, Wg]: xmaps = min(nrow, T) tiles to a row, ymaps = ceil(T / xmaps) rows, `padding` pixels of
    pad_value in front of every tile and behind the last; tile k at row (k // xmaps) (H + padding) + padding, column
    (k % xmaps) (W + padding) + padding.  A single tile comes back as it is, without a border."""
    T, _, H, W = tiles.shape
    if T == 1:
        return tiles[0].clone()
    xmaps = min(nrow, T)
    ymaps = -(-T // xmaps)
    grid = torch.full((3, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding), pad_value, dtype=torch.float32)
    for k in range(T):
        r0 = (k // xmaps) * (H + padding) + padding
        c0 = (k % xmaps) * (W + padding) + padding
        grid[:, r0:r0 + H, c0:c0 + W] = tiles[k]
    return grid


def quantise(grid):
    """[3, Hg, Wg] float32 -> [Hg, Wg, 3] uint8: times 255 rounded to float32, plus 0.5 rounded again, clamped to [0, 255],
    truncated.  A NaN gives 0 by definition (torch does not define the cast of a NaN)."""
    q = grid.clone().mul_(255)
    q.add_(0.5)
    q.clamp_(0, 255)
    q[torch.isnan(q)] = 0
    return q.permute(1, 2, 0).to(torch.uint8).contiguous()


def picture(tensors, nrow, padding=2, pad_value=0.0):
    """(float grid [3, Hg, Wg], uint8 image [Hg, Wg, 3]) of a list of tensors, each [n], [n, a], [n, a, b] or [n, c, h, w]; the
    tiles are the images of the first tensor, then of the second, ..."""
    data, _ = adapt_shape(dict(enumerate(tensors)))
    grid = make_grid(torch.cat(list(data.values())), nrow, padding, pad_value)
    return grid, quantise(grid)


def same_bits(a, b):
    """float32 tensors equal bit for bit (a NaN equals itself, +0 differs from -0)."""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and \
        torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
