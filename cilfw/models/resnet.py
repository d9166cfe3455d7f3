"""ResNet-18/34/50 backbones (NHWC) for the scale-out configs.

The reference repo only ships CIFAR ResNets; BASELINE.json's headline config is
ResNet-18 on CIFAR-100 and ResNet-50 on ImageNet-1000, so these are cilfw-native
additions. CIFAR inputs (<=64 px) get a 3x3/s1 stem with no max-pool; larger inputs
get the classic 7x7/s2 stem + 3x3/s2 max-pool. Projection ("option B") shortcuts:
1x1 conv + BN.

``ResNet.pod_tap`` is ``CifarResNet.pod_tap``'s counterpart: ``"pre"`` makes the
last block of each of the four stages take the unfused ``batchnorm_act`` +
``add_relu_tap`` tail in every pass, and ``return_maps`` then returns the sums
before each stage's last ReLU (the paper's POD tap) instead of the stage outputs.
"""

import torch.nn as nn

from ..ops import functional as CF
from .layers import Conv2d, BatchNormAct2d
from .resnet_cifar import POD_TAPS, run_stage_tapped


class BasicBlockB(nn.Module):
    expansion = 1

    def __init__(self, in_ch, out_ch, stride=1):
        super().__init__()
        self.conv1 = Conv2d(in_ch, out_ch, 3, stride=stride, padding=1)
        self.bn1 = BatchNormAct2d(out_ch, relu=True)
        self.conv2 = Conv2d(out_ch, out_ch, 3, stride=1, padding=1)
        self.bn2 = BatchNormAct2d(out_ch, relu=False)
        if stride != 1 or in_ch != out_ch:
            self.proj = Conv2d(in_ch, out_ch, 1, stride=stride, padding=0)
            self.proj_bn = BatchNormAct2d(out_ch, relu=False)
        else:
            self.proj = None

    def forward(self, x, tap=False):
        """``tap``: -> (y, z), the block output and its pre-ReLU sum."""
        out = self.bn1(self.conv1(x))
        residual = self.proj_bn(self.proj(x)) if self.proj is not None else x
        if tap:
            return self.bn2(self.conv2(out), residual, tap=True)
        return self.bn2(self.conv2(out), residual)  # fused bn+add+relu


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_ch, width, stride=1):
        super().__init__()
        out_ch = width * self.expansion
        self.conv1 = Conv2d(in_ch, width, 1, stride=1, padding=0)
        self.bn1 = BatchNormAct2d(width, relu=True)
        self.conv2 = Conv2d(width, width, 3, stride=stride, padding=1)
        self.bn2 = BatchNormAct2d(width, relu=True)
        self.conv3 = Conv2d(width, out_ch, 1, stride=1, padding=0)
        self.bn3 = BatchNormAct2d(out_ch, relu=False)
        if stride != 1 or in_ch != out_ch:
            self.proj = Conv2d(in_ch, out_ch, 1, stride=stride, padding=0)
            self.proj_bn = BatchNormAct2d(out_ch, relu=False)
        else:
            self.proj = None

    def forward(self, x, tap=False):
        """``tap``: -> (y, z), the block output and its pre-ReLU sum."""
        out = self.bn1(self.conv1(x))
        out = self.bn2(self.conv2(out))
        residual = self.proj_bn(self.proj(x)) if self.proj is not None else x
        if tap:
            return self.bn3(self.conv3(out), residual, tap=True)
        return self.bn3(self.conv3(out), residual)  # fused bn+add+relu


class ResNet(nn.Module):
    def __init__(self, block, layers, in_channels=3, small_input=True):
        super().__init__()
        self.small_input = small_input
        if small_input:
            self.stem = Conv2d(in_channels, 64, 3, stride=1, padding=1)
        else:
            self.stem = Conv2d(in_channels, 64, 7, stride=2, padding=3)
        # small_input: stem BN output feeds layer1's first conv AND its
        # identity skip — two consumers, so conv-side BN-backward fusion
        # could never be consumed (with a maxpool stem it is simply unused)
        self.stem_bn = BatchNormAct2d(64, relu=True, fuse_bwd=False)
        self.in_ch = 64
        self.layer1 = self._make_layer(block, 64, layers[0], stride=1)
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.out_dim = 512 * block.expansion
        self.pod_tap = "post"

    def _make_layer(self, block, width, n, stride):
        blocks = [block(self.in_ch, width, stride)]
        self.in_ch = width * block.expansion
        blocks += [block(self.in_ch, width, 1) for _ in range(n - 1)]
        return nn.Sequential(*blocks)

    def forward(self, x, return_maps=False):
        """-> (N, out_dim) features; with ``return_maps`` also the list of
        the four stage outputs (NHWC): post-ReLU, or with ``pod_tap == "pre"``
        each stage's sum before its last ReLU."""
        assert self.pod_tap in POD_TAPS, f"pod_tap {self.pod_tap!r}"
        x = self.stem_bn(self.stem(x))
        if not self.small_input:
            x = CF.max_pool(x, 3, 2, 1)
        if self.pod_tap == "pre":
            s1, z1 = run_stage_tapped(self.layer1, x)
            s2, z2 = run_stage_tapped(self.layer2, s1)
            s3, z3 = run_stage_tapped(self.layer3, s2)
            s4, z4 = run_stage_tapped(self.layer4, s3)
            feats = CF.global_avg_pool(s4)
            if return_maps:
                return feats, [z1, z2, z3, z4]
            return feats
        s1 = self.layer1(x)
        s2 = self.layer2(s1)
        s3 = self.layer3(s2)
        s4 = self.layer4(s3)
        feats = CF.global_avg_pool(s4)
        if return_maps:
            return feats, [s1, s2, s3, s4]
        return feats


def resnet18(small_input=True, **kw):
    return ResNet(BasicBlockB, [2, 2, 2, 2], small_input=small_input, **kw)


def resnet34(small_input=True, **kw):
    return ResNet(BasicBlockB, [3, 4, 6, 3], small_input=small_input, **kw)


def resnet50(small_input=False, **kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], small_input=small_input, **kw)
