"""`multivae/data/datasets/utils.py:10-47`: ResampleDataset — `dataset[sampler(dataset, idx)]`.

Here the sampler is an index tensor (what `MnistSvhn` needs): `base[index[i]]`.  The trainer's device-resident batch
iterator recognises it (`base`, `index`) and gathers `base.to(device)[index[batch]]` on the GPU instead of materialising
the resampled copy (5 x the paired MnistSvhn set would be 4 GB of host memory).

`multivae/data/datasets/utils.py:50-91`: adapt_shape — every modality of a dict as [n, 3, h, w] images of one common size, for
the pictures of metrics.Visualization and BaseTrainer.predict.  Those two hand the tensors as they are to kernels.image_grid, which
applies the same rules inside its one launch; adapt_shape is the public helper and the plain-torch path."""
from math import ceil, floor

import torch
import torch.nn.functional as F


def as_image_batch(t):
    """[n], [n, a], [n, a, b] -> [n, 1, 1, 1], [n, 1, 1, a], [n, 1, a, b] (views); a 4-d tensor as it is."""
    while t.dim() < 4:
        t = t.unsqueeze(1)
    if t.dim() != 4:
        raise AttributeError("Can't visualize data with more than 3 dimensions")
    return t


def adapt_shape(data):
    """`data` with every tensor brought to [n_data, 3, h, w], h and w the largest height and width over the modalities, and the
    shape (3, h, w).  One channel is replicated, two get a third of zeros, of more the first three are kept; a smaller image is
    centred in zeros (floor of the difference in front, ceil behind).  The dict is changed in place, as in the reference; every
    tensor stays on its device (the reference's CPU zeros for the two-channel case fail on a GPU tensor)."""
    for m in data:
        x = as_image_batch(data[m])
        if x.shape[1] == 1:
            x = torch.cat([x, x, x], dim=1)
        elif x.shape[1] == 2:
            n, _, h, w = x.shape
            x = torch.cat([x, torch.zeros(n, 1, h, w, dtype=x.dtype, device=x.device)], dim=1)
        else:
            x = x[:, :3, :, :]
        data[m] = x
    h = max(data[m].shape[2] for m in data)
    w = max(data[m].shape[3] for m in data)
    for m in data:
        hm, wm = data[m].shape[2:]
        data[m] = F.pad(data[m], (floor((w - wm) / 2), ceil((w - wm) / 2), floor((h - hm) / 2), ceil((h - hm) / 2)),
                        mode="constant", value=0)
    return data, (3, h, w)


class ResampleDataset(torch.utils.data.Dataset):
    def __init__(self, base: torch.Tensor, index: torch.Tensor, transform=None):
        self.base = base
        self.index = torch.as_tensor(index, dtype=torch.long)
        self.transform = transform

    def __len__(self):
        return len(self.index)

    def __getitem__(self, idx):
        i = self.index[idx]
        if torch.is_tensor(i) and i.numel() and (int(i.min()) < 0 or int(i.max()) >= len(self.base)):
            raise IndexError("out of range")
        x = self.base[i]
        return self.transform(x) if self.transform is not None else x
