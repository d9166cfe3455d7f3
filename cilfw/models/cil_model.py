"""CilModel / CilClassifier — dynamic multi-head classifier + WA weight alignment.

Capability parity with reference template.py:87-166:
- CilClassifier: one linear head appended per task (adaption, template.py:103-104);
  forward = concatenation of all head logits in head order (template.py:99-101).
  cilfw computes it as ONE fused GEMM over the row-concatenated head weights instead
  of the reference's per-head GEMM + torch.cat.
- CilModel.forward -> (logits, features) (template.py:120-123); extract_vector
  (:117); copy (:125); freeze (:128-144); prev_model_adaption (:146-150);
  after_model_adaption -> weight_align (:152-166).
- weight_align: gamma = mean(||w_old rows||) / mean(||w_new rows||), rescales the
  NEWEST head's weight in place (the core WA step, template.py:156-166).
- CosineClassifier (``CilModel(..., head="cosine")``): the cosine-normalised
  head of LUCIR / PODNet, the other standard answer to the old-versus-new bias;
  no reference counterpart.
"""

import copy as _copy

import torch
import torch.nn as nn

from ..ops import functional as CF
from ..ops import cosine as COS
from ..ops import lsc as LSC
from . import resnet_cifar, resnet


def get_backbone(name, input_size=32):
    """Backbone factory (reference template.py:72-84 + BASELINE scale-out models)."""
    small = input_size <= 64
    factories = {
        "resnet20": lambda: resnet_cifar.resnet20(),
        "resnet32": lambda: resnet_cifar.resnet32(),
        "resnet44": lambda: resnet_cifar.resnet44(),
        "resnet56": lambda: resnet_cifar.resnet56(),
        "resnet110": lambda: resnet_cifar.resnet110(),
        "resnet18": lambda: resnet.resnet18(small_input=small),
        "resnet34": lambda: resnet.resnet34(small_input=small),
        "resnet50": lambda: resnet.resnet50(small_input=small),
    }
    if name not in factories:
        raise NotImplementedError(f"unknown backbone {name!r}")
    return factories[name]()


class CilClassifier(nn.Module):
    """Growable multi-head linear classifier; logits = [head_0 | head_1 | ...]."""

    def __init__(self, embed_dim, nb_classes):
        super().__init__()
        self.embed_dim = embed_dim
        self.heads = nn.ModuleList()
        self.adaption(nb_classes)

    def adaption(self, nb_new_classes):
        head = nn.Module()
        head.weight = nn.Parameter(torch.empty(nb_new_classes, self.embed_dim))
        nn.init.kaiming_normal_(head.weight)
        head.bias = nn.Parameter(torch.zeros(nb_new_classes))
        head.out_features = nb_new_classes
        self.heads.append(head)

    @property
    def nb_classes(self):
        return sum(h.out_features for h in self.heads)

    def forward(self, x):
        # one fused GEMM over concatenated head weights (heads are tiny:
        # C x 64..2048); frozen models use a cached concatenation
        cat = getattr(self, "_frozen_cat", None)
        if cat is not None:
            return CF.linear(x, cat[0], cat[1])
        w = torch.cat([h.weight for h in self.heads], dim=0)
        b = torch.cat([h.bias for h in self.heads], dim=0)
        return CF.linear(x, w, b)

    def __getitem__(self, i):
        return self.heads[i]

    def __len__(self):
        return len(self.heads)


class CosineClassifier(nn.Module):
    """Growable cosine-normalised classifier (LUCIR; PODNet's LSC head with
    one proxy per class): logits = sigma * cos(feature, class weight), heads
    concatenated in head order. No bias; ONE scale ``sigma`` shared by all
    heads and trained like any other parameter. Rescaling a weight row cannot
    change a logit, so no weight alignment applies.

    ``nb_proxy = K > 1`` is PODNet's full LSC head: a head for ``n`` classes
    holds ``weight (n K, D)``, class-major (class ``c``'s proxies are rows
    ``c K .. c K + K - 1``), ``out_features`` stays ``n``, and the ``K``
    cosines of a class are reduced by ``ops.lsc_reduce`` (their
    softmax(``proxy_gamma`` cosine)-weighted mean, times ``sigma``)."""

    def __init__(self, embed_dim, nb_classes, scale_init=1.0, nb_proxy=1,
                 proxy_gamma=1.0):
        super().__init__()
        if not 1 <= int(nb_proxy) <= LSC.MAX_PROXY:
            raise ValueError(f"nb_proxy must be in 1..{LSC.MAX_PROXY} "
                             f"(got {nb_proxy})")
        if not float(proxy_gamma) >= 0:
            raise ValueError(f"proxy_gamma must be >= 0 (got {proxy_gamma})")
        self.embed_dim = embed_dim
        self.nb_proxy = int(nb_proxy)
        self.proxy_gamma = float(proxy_gamma)
        self.heads = nn.ModuleList()
        self.sigma = nn.Parameter(torch.full((1,), float(scale_init)))
        if self.nb_proxy > 1:
            # the scale of the pure cosines that lsc_reduce reads: not
            # trained, not part of the state dict
            self.register_buffer("unit_scale", torch.ones(1),
                                 persistent=False)
        self.adaption(nb_classes)

    def adaption(self, nb_new_classes):
        head = nn.Module()
        head.weight = nn.Parameter(torch.empty(
            nb_new_classes * self.nb_proxy, self.embed_dim))
        nn.init.kaiming_normal_(head.weight)
        head.out_features = nb_new_classes
        self.heads.append(head)

    @property
    def nb_classes(self):
        return sum(h.out_features for h in self.heads)

    def forward(self, x):
        # one cosine_linear over the row-concatenated fp32 masters; a frozen
        # model uses its cached normalised rows (cast_compute_weights_)
        cat = getattr(self, "_frozen_cat", None)
        if self.nb_proxy > 1:
            # pure cosines against all n K proxies, then the per-class reduce
            if cat is not None:
                with torch.no_grad():
                    sims = COS.cosine_linear_frozen(x, cat[0], cat[2])
                    return LSC.lsc_reduce(sims, cat[1], self.nb_proxy,
                                          self.proxy_gamma)
            w = torch.cat([h.weight for h in self.heads], dim=0)
            sims = COS.cosine_linear(x, w, self.unit_scale)
            return LSC.lsc_reduce(sims, self.sigma, self.nb_proxy,
                                  self.proxy_gamma)
        if cat is not None:
            return COS.cosine_linear_frozen(x, cat[0], cat[1])
        w = torch.cat([h.weight for h in self.heads], dim=0)
        return COS.cosine_linear(x, w, self.sigma)

    def __getitem__(self, i):
        return self.heads[i]

    def __len__(self):
        return len(self.heads)


HEAD_KINDS = ("linear", "cosine")


class CilModel(nn.Module):
    def __init__(self, backbone_name, input_size=32, head="linear",
                 cos_scale_init=1.0, nb_proxy=1, proxy_gamma=1.0,
                 pod_tap="post"):
        super().__init__()
        if pod_tap not in resnet_cifar.POD_TAPS:
            raise ValueError(f"unknown pod_tap {pod_tap!r} (one of "
                             f"{resnet_cifar.POD_TAPS})")
        if head not in HEAD_KINDS:
            raise ValueError(f"unknown head kind {head!r} (one of "
                             f"{HEAD_KINDS})")
        if int(nb_proxy) != 1 and head != "cosine":
            raise ValueError(f"nb_proxy = {nb_proxy} needs a cosine head "
                             f"(got head {head!r})")
        self.nb_proxy = int(nb_proxy)
        self.proxy_gamma = float(proxy_gamma)
        self.backbone = get_backbone(backbone_name, input_size)
        # "pre": return_maps gives each stage's sum before its last ReLU (the
        # paper's POD tap); a copy() of the model, the teacher, inherits it
        self.backbone.pod_tap = pod_tap
        self.head_kind = head
        self.cos_scale_init = cos_scale_init
        self.fc = None

    @property
    def feature_dim(self):
        return self.backbone.out_dim

    def extract_vector(self, x):
        return self.backbone(x)

    def forward(self, x, return_maps=False):
        """-> (logits, features); with ``return_maps`` -> (logits, features,
        maps), maps = the backbone's stage maps (for ops.pod_loss): the stage
        outputs, or with ``pod_tap="pre"`` their pre-ReLU sums."""
        if return_maps:
            features, maps = self.backbone(x, return_maps=True)
            return self.fc(features), features, maps
        features = self.backbone(x)
        logits = self.fc(features)
        return logits, features

    def copy(self):
        return _copy.deepcopy(self)

    def freeze(self, names=("all",)):
        """Freeze submodules by name; 'all' freezes everything and sets eval
        (reference template.py:128-144)."""
        freezed = []
        for name in names:
            if name == "all":
                for p in self.parameters():
                    p.requires_grad = False
                self.eval()
                return ["all"]
            if hasattr(self, name):
                freezed.append(name)
                mod = getattr(self, name)
                for p in mod.parameters():
                    p.requires_grad = False
                mod.eval()
        missing = set(names) - set(freezed)
        if missing:
            raise AttributeError(f"unknown submodules to freeze: {missing}")
        return freezed

    @torch.no_grad()
    def cast_compute_weights_(self, dtype):
        """Convert conv/linear weights to the compute dtype in place — used on
        the FROZEN teacher so its forward skips the per-step fp32->bf16 casts
        (the fp32 masters only matter for models that train). Also precomputes
        each BN's eval (mean, invstd) so the per-call finalize launch is
        skipped (the running stats of a frozen model never change)."""
        from .layers import Conv2d, BatchNormAct2d
        for m in self.modules():
            if isinstance(m, Conv2d):
                m.weight.data = m.weight.data.to(dtype)
            elif isinstance(m, BatchNormAct2d):
                mean = m.running_mean.float().clone()
                invstd = torch.rsqrt(m.running_var.float() + m.eps)
                m.running_mean._cilfw_frozen = (mean.contiguous(),
                                                invstd.contiguous())
        if isinstance(self.fc, CosineClassifier):
            # the normalisation reads the fp32 masters, which stay as they
            # are; the unit rows (the GEMM operand) and sigma are cached once,
            # so a frozen head costs one rownorm_fwd on the features + the GEMM
            w = torch.cat([h.weight for h in self.fc.heads], 0).float()
            self.fc._frozen_cat = (
                COS.cosine_normalize_weights(w).to(dtype).contiguous(),
                self.fc.sigma.detach().float().clone())
            if self.fc.nb_proxy > 1:
                self.fc._frozen_cat += (
                    self.fc.unit_scale.detach().float().clone(),)
        elif self.fc is not None:
            for h in self.fc.heads:
                h.weight.data = h.weight.data.to(dtype)
                h.bias.data = h.bias.data.to(dtype)
            self.fc._frozen_cat = (
                torch.cat([h.weight for h in self.fc.heads], 0).contiguous(),
                torch.cat([h.bias for h in self.fc.heads], 0).contiguous())
        return self

    def prev_model_adaption(self, nb_classes):
        if self.fc is None:
            if self.head_kind == "cosine":
                self.fc = CosineClassifier(self.feature_dim, nb_classes,
                                           self.cos_scale_init,
                                           self.nb_proxy, self.proxy_gamma)
            else:
                self.fc = CilClassifier(self.feature_dim, nb_classes)
        else:
            self.fc.adaption(nb_classes)
        # keep the new head on the model's device/dtype
        ref = next(self.backbone.parameters())
        self.fc.to(ref.device)

    def after_model_adaption(self, nb_classes, args=None):
        task_id = getattr(args, "task_id", len(self.fc) - 1) if args is not None \
            else len(self.fc) - 1
        if task_id > 0:
            if self.head_kind == "cosine":
                print("cosine head: weight aligning skipped (rescaling a "
                      "weight row cannot change a cosine logit)")
                return
            self.weight_align(nb_classes)

    @torch.no_grad()
    def imprint_new_head(self, protos):
        """LUCIR's class-mean imprinting: ``protos (n_new, D)`` are the
        unit-norm class prototypes of the newest head's classes in class
        order (``ops.nme_prototypes``); its weight rows become ``p_c *
        mean(|w_old rows|_2)``. -> (rows set, mean old norm)."""
        if self.head_kind != "cosine":
            raise RuntimeError(
                "imprint_new_head: imprinting sets the rows of a cosine head "
                f"(this model has a {self.head_kind} head)")
        if self.fc is None or len(self.fc) < 2:
            raise RuntimeError(
                "imprint_new_head: needs at least one old head to take the "
                "mean row norm from")
        if self.fc.nb_proxy > 1:
            raise RuntimeError(
                "imprint_new_head: a head with nb_proxy > 1 cannot be "
                "imprinted (identical proxies would never separate)")
        new = self.fc.heads[-1].weight
        if protos.dim() != 2 or tuple(protos.shape) != tuple(new.shape):
            raise ValueError(
                f"imprint_new_head: {tuple(protos.shape)} prototypes for a "
                f"new head of shape {tuple(new.shape)}")
        w_old = torch.cat([h.weight for h in self.fc.heads[:-1]], dim=0)
        norm_old = torch.norm(w_old.float(), p=2, dim=1).mean()
        new.copy_((protos.to(new.device).float() * norm_old).to(new.dtype))
        return new.shape[0], norm_old.item()

    @torch.no_grad()
    def init_new_proxies(self, proxies):
        """PODNet's k-means initialisation of a multi-proxy head: ``proxies
        (n_new * nb_proxy, D)`` are the unit-norm k-means centres of the
        newest head's classes, class-major (``ops.kmeans_proxies``); its
        weight rows become ``proxies * mean(|w_old rows|_2)``. -> (rows set,
        mean old norm)."""
        if self.head_kind != "cosine":
            raise RuntimeError(
                "init_new_proxies: proxies are the rows of a cosine head "
                f"(this model has a {self.head_kind} head)")
        if self.fc is None or len(self.fc) < 2:
            raise RuntimeError(
                "init_new_proxies: needs at least one old head to take the "
                "mean row norm from")
        if self.fc.nb_proxy == 1:
            raise RuntimeError(
                "init_new_proxies: a head with nb_proxy = 1 has one row per "
                "class; set it to the class mean with imprint_new_head")
        new = self.fc.heads[-1].weight
        if proxies.dim() != 2 or tuple(proxies.shape) != tuple(new.shape):
            raise ValueError(
                f"init_new_proxies: {tuple(proxies.shape)} proxies for a "
                f"new head of shape {tuple(new.shape)} (classes x nb_proxy = "
                f"{self.fc.nb_proxy} rows)")
        w_old = torch.cat([h.weight for h in self.fc.heads[:-1]], dim=0)
        norm_old = torch.norm(w_old.float(), p=2, dim=1).mean()
        new.copy_((proxies.to(new.device).float() * norm_old).to(new.dtype))
        return new.shape[0], norm_old.item()

    @torch.no_grad()
    def weight_align(self, nb_new_classes):
        """WA: rescale the newest head so mean new-row norm == mean old-row norm."""
        if self.head_kind == "cosine":
            raise RuntimeError(
                "weight_align: a cosine head has no row norms to align "
                "(its logits are invariant under rescaling a weight row)")
        w = torch.cat([h.weight for h in self.fc.heads], dim=0)
        norms = torch.norm(w, p=2, dim=1)
        norm_old = norms[:-nb_new_classes]
        norm_new = norms[-nb_new_classes:]
        gamma = norm_old.mean() / norm_new.mean()
        print(f"old norm: {norm_old.mean().item():.4f}, "
              f"new norm: {norm_new.mean().item():.4f}, gamma: {gamma.item():.4f}")
        self.fc.heads[-1].weight.mul_(gamma)
        return gamma.item()


def freeze_parameters(m, requires_grad=False):
    """reference template.py:61-69."""
    if isinstance(m, nn.Parameter):
        m.requires_grad = requires_grad
    else:
        for p in m.parameters():
            p.requires_grad = requires_grad
