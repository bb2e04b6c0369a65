"""`multivae/metrics/classifiers/mmnist.py`: the PolyMNIST digit classifier and the loader of its five pretrained copies.

The architecture is fixed (3x28x28 -> conv 4x4/s2 (10) -> conv 4x4/s2 (20) -> 980 -> 128 -> 10, dropout after the first three layers),
and the coherence evaluation runs it on every generated image, so in eval mode on the GPU the whole network is ONE launch of
csrc/clf.hip (`kernels.polyclf_forward`), which can also hand back the argmax or add straight into a `ClassCounts` table.  The
module keeps the reference's layout (`encoder` is an nn.Sequential, state-dict keys encoder.0 / 3 / 7 / 10), so its checkpoints load
unchanged, and the kernel reads the parameters in place.  Training, the CPU, other dtypes and anything autograd has to record run the
torch modules, as models/nn/flows.py does."""
import os

import torch
from torch import nn


class Flatten(nn.Module):
    """[n, ...] -> [n, -1]."""

    def forward(self, x):
        return x.reshape(x.shape[0], -1)


class ClassifierPolyMNIST(nn.Module):
    """PolyMNIST classifier: logits [n, 10] of images [n, 3, 28, 28]."""

    def __init__(self):
        super().__init__()
        self.encoder = nn.Sequential(
            nn.Conv2d(3, 10, kernel_size=4, stride=2, padding=1),   # 0: [10, 14, 14]
            nn.Dropout2d(0.5),
            nn.ReLU(),
            nn.Conv2d(10, 20, kernel_size=4, stride=2, padding=1),  # 3: [20, 7, 7]
            nn.Dropout2d(0.5),
            nn.ReLU(),
            Flatten(),
            nn.Linear(980, 128),                                    # 7
            nn.Dropout(0.5),
            nn.ReLU(),
            nn.Linear(128, 10),                                     # 10
        )

    def kernel_params(self):
        """The eight parameters in the order of mvk_polyclf_fwd."""
        e = self.encoder
        return [e[0].weight, e[0].bias, e[3].weight, e[3].bias, e[7].weight, e[7].bias, e[10].weight, e[10].bias]

    def kernel_ok(self, x):
        """Whether the kernel can classify x: eval mode (dropout is the identity), a CUDA fp32 [n,3,28,28] tensor."""
        if self.training or not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32:
            return False
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, 28, 28):
            return False
        params = self.kernel_params()
        return not any(p.device != x.device or p.dtype != torch.float32 or not p.is_contiguous() for p in params)

    def fused_ok(self, x):
        """Whether forward(x) takes the fused launch: `kernel_ok`, and nothing for autograd to record in the logits."""
        if not self.kernel_ok(x):
            return False
        return not torch.is_grad_enabled() or not (x.requires_grad or any(p.requires_grad for p in self.kernel_params()))

    def forward(self, x):
        if self.fused_ok(x):
            from ... import kernels

            return kernels.polyclf_forward(x.contiguous(), [p.detach() for p in self.kernel_params()])
        return self.encoder(x)

    def classify(self, x, pred=None, labels=None, counts=None):
        """The outputs of the fused launch other than the logits, for an x that is `kernel_ok` (integers: there is nothing for
        autograd in them): pred [n] int32 is filled with the argmax, counts [11, 2] int64 (ClassCounts.counts) accumulates the
        (correct, count) pairs under labels[i % len(labels)] (1-d int64).  With neither given, pred is allocated.  Returns pred
        (None when only counts were asked for)."""
        if not self.kernel_ok(x):
            raise ValueError("ClassifierPolyMNIST.classify runs the fused kernel only: eval mode, a CUDA float32 [n,3,28,28] tensor")
        from ... import kernels

        if pred is None and counts is None:
            pred = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
        params = [p.detach() for p in self.kernel_params()]
        kernels.polyclf_forward(x.detach().contiguous(), params, pred=pred, labels=labels, counts=counts)
        return pred


def load_mmnist_classifiers(data_path=".data/clf", device="cpu"):
    """The five pretrained classifiers {"m0": ..., "m4": ...} from the state dicts data_path/pretrained_img_to_digit_clf_m{i} (the
    `clf` folder that comes with the PolyMNIST data).  Nothing is fetched."""
    clfs = {}
    for i in range(5):
        clf = ClassifierPolyMNIST()
        clf.load_state_dict(torch.load(os.path.join(data_path, f"pretrained_img_to_digit_clf_m{i}"), map_location=torch.device(device)))
        clfs[f"m{i}"] = clf.to(device)
    return clfs
