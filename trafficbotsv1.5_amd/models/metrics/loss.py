"""`AngularError` / `BalancedKL` with the reference's interfaces (models/metrics/loss.py:9-77): the scalar glue of the training
loss. The reward's heading term inside a rollout is tbx_sim_step's / tbx_train_chain's (the default, cosine) or tbx_il_reward_fwd's over
the finished log (every other angular type); these classes serve callers that hold tensors (a few hundred elements, once per batch -
SURVEY 8a rows 18-19: negligible)."""
import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.distributions import Independent, Normal, OneHotCategoricalStraightThrough, kl_divergence

from ... import abi
from ..modules.distributions import one_hot_categorical

# the criteria of an imitation term by the reference's names (torch.nn classes with reduction="none") as torch expressions of
# (input, target): what the torch state machine of the training step differentiates, and the CPU path of the classes below.
# HuberLoss() at delta = 1 is SmoothL1Loss() at beta = 1, value and gradient.
TORCH_CRITERIA = {"SmoothL1Loss": lambda a, b: F.smooth_l1_loss(a, b, reduction="none"), "MSELoss": lambda a, b: F.mse_loss(a, b, reduction="none"),
                  "L1Loss": lambda a, b: F.l1_loss(a, b, reduction="none"), "HuberLoss": lambda a, b: F.huber_loss(a, b, reduction="none")}


def criterion_code(name: str, what: str) -> int:
    """TBX_IL_* of a criterion name; any other name: NotImplementedError listing the accepted ones."""
    if name not in abi.IL_CRITERIA:
        raise NotImplementedError(f"{what}: criterion {name!r} is not implemented; accepted: {', '.join(abi.IL_CRITERIA)}")
    return abi.IL_CRITERIA[name]


def cast_rad(angle: Tensor) -> Tensor:
    """utils/transform_utils.py:9-11: into [-pi, pi)."""
    return (angle + math.pi) % (2 * math.pi) - math.pi


class AngularError:
    """models/metrics/loss.py:9-36: the error of two angles by `angular_type` - None (the criterion on the raw difference), "cast" (on
    the difference wrapped into [-pi, pi)), "cosine" (0.5 (1 - cos); the criterion is not looked up, as in the reference) or "vector" (the
    criterion on the cosines plus on the sines). Device tensors outside autograd go through tbx_il_reward_fwd (a one-step log with only
    the rotation term); CPU tensors, and tensors that carry a gradient, through the torch expression `compute_torch`."""

    def __init__(self, criterion: str, angular_type: Optional[str]) -> None:
        if angular_type not in abi.IL_ANGULAR:
            raise NotImplementedError(f"AngularError: angular_type {angular_type!r} is not implemented; accepted: null, cast, cosine, vector")
        self.angular_type, self.angular_code = angular_type, abi.IL_ANGULAR[angular_type]
        self.criterion_code = abi.IL_CRITERIA.get(criterion, abi.IL_SMOOTH_L1) if angular_type == "cosine" else criterion_code(criterion, "AngularError")
        self.criterion = None if angular_type == "cosine" else TORCH_CRITERIA[criterion]

    def compute_torch(self, preds: Tensor, target: Tensor) -> Tensor:
        if self.angular_type is None:
            return self.criterion(preds, target)
        if self.angular_type == "cast":
            diff_angle = cast_rad(preds - target)
            return self.criterion(diff_angle, torch.zeros_like(diff_angle))
        if self.angular_type == "cosine":
            return 0.5 * (1 - torch.cos(preds - target))
        return self.criterion(torch.cos(preds), torch.cos(target)) + self.criterion(torch.sin(preds), torch.sin(target))

    def compute(self, preds: Tensor, target: Tensor) -> Tensor:
        if not (preds.is_cuda and target.is_cuda) or preds.dtype != torch.float32 or target.dtype != torch.float32 or (
                torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad)) or preds.numel() == 0:
            return self.compute_torch(preds, target)
        from ... import hip

        # criterion(preds, target): preds in the ground truth's place, target in the prediction's (d = gt - pred); weight -1: r_rot = e_rot
        preds, target = torch.broadcast_tensors(preds, target)
        n = preds.numel()
        pose = lambda x: torch.cat([torch.zeros(n, 2, dtype=torch.float32, device=x.device), x.reshape(n, 1)], 1)
        ones, zeros = torch.ones(1, 1, n, dtype=torch.uint8, device=preds.device), torch.zeros(1, 1, n, 3, dtype=torch.float32, device=preds.device)
        e = hip.il_reward_fwd(ones, pose(target).view(1, 1, n, 3), zeros, ones.view(1, n, 1), pose(preds).view(1, n, 1, 3), zeros.view(1, n, 1, 3),
                              (abi.IL_SMOOTH_L1, self.criterion_code, abi.IL_SMOOTH_L1, self.angular_code), (0.0, -1.0, 0.0), gt_offset=0)
        return e.view(preds.shape)


def detached(d: Independent) -> Independent:
    """A latent distribution (Independent over Normal or over the one-hot categorical) without its graph (loss.py:59-66): the Normal from
    its detached loc / scale, the categorical from its detached probabilities."""
    b = d.base_dist
    if isinstance(b, Normal):
        return Independent(Normal(b.loc.detach(), b.scale.detach(), validate_args=False), 1, validate_args=False)
    return one_hot_categorical(probs=b.probs.detach())


class BalancedKL:
    """Dreamer-v2 KL balancing (loss.py:39-77) of two latent distributions of one family: diagonal Gaussians (latent_encoder std_gaus /
    diag_gaus) or multi-categoricals (std_cat / cat). A pair of different families: ValueError."""

    def __init__(self, kl_balance_scale: float, kl_free_nats: float) -> None:
        self.alpha, self.free_nats = kl_balance_scale, kl_free_nats

    def compute(self, posterior: Independent, prior: Independent) -> Tensor:
        fam = lambda d: Normal if isinstance(d.base_dist, Normal) else (
            OneHotCategoricalStraightThrough if isinstance(d.base_dist, OneHotCategoricalStraightThrough) else None)
        if fam(posterior) is None or fam(posterior) is not fam(prior):
            raise ValueError(f"BalancedKL: posterior {type(posterior.base_dist).__name__} and prior {type(prior.base_dist).__name__} "
                             f"must both be Normal or both be OneHotCategoricalStraightThrough")
        if self.alpha > 0:
            e0, e1 = kl_divergence(detached(posterior), prior), kl_divergence(posterior, detached(prior))
            if self.free_nats > 0:
                e0, e1 = torch.clamp(e0, min=self.free_nats), torch.clamp(e1, min=self.free_nats)
            return e0 + self.alpha * e1
        e = kl_divergence(posterior, prior)
        return torch.clamp(e, min=self.free_nats) if self.free_nats > 0 else e
