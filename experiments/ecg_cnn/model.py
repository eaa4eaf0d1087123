"""ecg_cnn task: 1-D CNN + LSTM + attention heartbeat classifier.

Reference: experiments/ecg_cnn/model.py:14-178 (conv-skip blocks with
Swish, bidirectional-style LSTM readout, linear attention pooling; 5 MIT-BIH
heartbeat classes over 187-sample beats).  This implementation keeps the
same topology but outputs logits (the reference applies softmax inside
``forward`` and then cross-entropy on probabilities — a quirk we do not
reproduce) and shows the custom-metric contract with a macro-F1.
"""

import torch
from torch import nn
from torch.nn import functional as F

from msrflute_amd.core.model import BaseModel
from msrflute_amd.ops.lstm import FusedLSTM
from msrflute_amd.utils import to_device


class ConvSkipBlock(nn.Module):
    """Three 1-D convs with BatchNorm + SiLU (=Swish), a 1x1 skip, maxpool."""

    def __init__(self, in_ch, out_ch, kernel=5):
        super().__init__()
        pad = kernel // 2
        self.conv1 = nn.Conv1d(in_ch, out_ch, kernel, padding=pad)
        self.conv2 = nn.Conv1d(out_ch, out_ch, kernel, padding=pad)
        self.conv3 = nn.Conv1d(out_ch, out_ch, kernel, padding=pad)
        self.bn1 = nn.BatchNorm1d(out_ch)
        self.bn2 = nn.BatchNorm1d(out_ch)
        self.bn3 = nn.BatchNorm1d(out_ch)
        self.skip = nn.Conv1d(in_ch, out_ch, 1)
        self.pool = nn.MaxPool1d(2)

    def forward(self, x):
        h = F.silu(self.bn1(self.conv1(x)))
        h = F.silu(self.bn2(self.conv2(h)))
        h = self.bn3(self.conv3(h) + self.skip(x))
        return self.pool(F.silu(h))


class ECGNet(nn.Module):
    def __init__(self, input_size=1, hid_size=256, n_classes=5,
                 kernel_size=5, lstm_hidden=64):
        super().__init__()
        self.conv1 = ConvSkipBlock(input_size, hid_size, kernel_size)
        self.conv2 = ConvSkipBlock(hid_size, hid_size // 2, kernel_size)
        # nn.LSTM's parameter names and init draws; on the GPU the fused
        # recurrence kernels (hidden 64: W_hh in registers), nn.LSTM on CPU
        self.lstm = FusedLSTM(hid_size // 2, lstm_hidden)
        self.attn = nn.Linear(lstm_hidden, lstm_hidden, bias=False)
        self.fc = nn.Linear(lstm_hidden, n_classes)

    def forward(self, x):
        if x.dim() == 2:
            x = x.unsqueeze(1)  # [B, 187] -> [B, 1, 187]
        h = self.conv2(self.conv1(x))          # [B, C, T/4]
        seq, _ = self.lstm(h.transpose(1, 2))  # [B, T/4, H]
        scores = torch.softmax(self.attn(seq), dim=1)
        pooled = (scores * seq).sum(dim=1)     # attention pooling
        return self.fc(pooled)


def macro_f1(pred: torch.Tensor, target: torch.Tensor, n_classes: int) -> float:
    f1s = []
    for c in range(n_classes):
        tp = ((pred == c) & (target == c)).sum().item()
        fp = ((pred == c) & (target != c)).sum().item()
        fn = ((pred != c) & (target == c)).sum().item()
        if tp + fp + fn == 0:
            continue
        f1s.append(2 * tp / (2 * tp + fp + fn))
    return sum(f1s) / len(f1s) if f1s else 0.0


class SuperNet(BaseModel):
    def __init__(self, model_config):
        super().__init__()
        self.n_classes = model_config.get("n_classes", 5)
        self.net = ECGNet(
            input_size=model_config.get("input_size", 1),
            hid_size=model_config.get("hid_size", 256),
            n_classes=self.n_classes,
            kernel_size=model_config.get("kernel_size", 5))

    def loss(self, input):
        x, y = to_device(input["x"]), to_device(input["y"])
        return F.cross_entropy(self.net(x), y.long())

    def inference(self, input):
        x, y = to_device(input["x"]), to_device(input["y"])
        output = self.net(x)
        pred = torch.argmax(output, dim=1)
        acc = (pred == y).float().mean().item()
        return {"output": output, "acc": acc, "batch_size": x.shape[0],
                "f1_macro": {"value": macro_f1(pred, y, self.n_classes),
                             "higher_is_better": True}}
