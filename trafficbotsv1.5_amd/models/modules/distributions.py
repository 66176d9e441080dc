"""Distribution wrappers with the reference's interface (modules/distributions.py): thin torch.distributions
holders, used once per batch (latent / destination sampling), never inside the per-step loop."""
from typing import Optional, Union

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.distributions import Categorical, Distribution, Independent, Normal, OneHotCategoricalStraightThrough


class MyDist:
    distribution = None
    valid: Optional[Tensor] = None


class DiagGaussian(MyDist):
    def __init__(self, mean: Tensor, log_std: Tensor, valid: Optional[Tensor] = None) -> None:
        self.mean, self.valid = mean, valid
        self.distribution = Independent(Normal(mean, log_std.exp(), validate_args=False), 1, validate_args=False)
        self.stddev = self.distribution.stddev

    def log_prob(self, sample: Tensor) -> Tensor:
        return self.distribution.log_prob(sample)

    def sample(self, deterministic: Union[bool, Tensor]) -> Tensor:
        if isinstance(deterministic, Tensor):
            d = deterministic.unsqueeze(-1)
            return self.distribution.mean.masked_fill(~d, 0) + self.distribution.rsample().masked_fill(d, 0)
        return self.distribution.mean if deterministic else self.distribution.rsample()

    def repeat_interleave_(self, repeats: int, dim: int) -> None:
        self.mean = self.mean.repeat_interleave(repeats, dim)
        self.stddev = self.stddev.repeat_interleave(repeats, dim)
        self.distribution = Independent(Normal(self.mean, self.stddev, validate_args=False), 1, validate_args=False)
        if self.valid is not None:
            self.valid = self.valid.repeat_interleave(repeats, dim)


def one_hot_categorical(logits: Optional[Tensor] = None, probs: Optional[Tensor] = None) -> Independent:
    """Independent(OneHotCategoricalStraightThrough(...), 1) without argument validation. torch hands `validate_args` to the outer object
    only: the Categorical inside is built with the class default and would check its arguments (and later every sample) with a host read - not allowed here, and
    an error inside a captured step. The default is switched off around the construction and put back."""
    prev = Distribution._validate_args
    Distribution.set_default_validate_args(False)
    try:
        d = Independent(OneHotCategoricalStraightThrough(probs=probs, logits=logits, validate_args=False), 1, validate_args=False)
    finally:
        Distribution.set_default_validate_args(prev)
    d.base_dist._categorical._validate_args = False  # (its log_prob would otherwise validate the sample: the same host read)
    return d


class MultiCategorical(MyDist):
    """distributions.py:67-120: n_cat independent one-hot categoricals of n_class classes per agent; a sample is the n_cat one-hot
    vectors flattened to [.., n_cat * n_class]. A random sample is the Gumbel-max of the logits, argmax(logits - log(-log u)) with u
    uniform in (0, 1) (ties to the lowest class), as a straight-through value one_hot + probs - probs.detach(): the value of the
    one-hot, the gradient of the probabilities. u is `noise` (the logits' shape) or drawn from the generator of the logits' device;
    nothing is read back on the host."""

    def __init__(self, logits: Tensor, valid: Optional[Tensor] = None) -> None:
        self._set(logits)
        self.valid = valid

    def _set(self, logits: Tensor) -> None:
        self.logits = logits
        self.distribution = one_hot_categorical(logits=logits)
        self.n_cat, self.n_class, self._dtype = logits.shape[-2], logits.shape[-1], logits.dtype

    @property
    def probs(self) -> Tensor:
        return self.distribution.base_dist.probs

    def log_prob(self, sample: Tensor) -> Tensor:
        return self.distribution.log_prob(sample.view(*sample.shape[:-1], self.n_cat, self.n_class))

    def _one_hot(self, score: Tensor) -> Tensor:  # (argmax returns the first of equal maxima on both devices)
        return F.one_hot(score.argmax(-1), num_classes=self.n_class).type(self._dtype)

    def _rnd(self, noise: Optional[Tensor]) -> Tensor:
        u = noise
        if u is None:  # (0, 1): rand() is in [0, 1), so its zeros move to the smallest positive step
            u = torch.rand(self.logits.shape, dtype=self._dtype, device=self.logits.device).clamp_(min=torch.finfo(self._dtype).tiny)
        probs = self.probs
        return self._one_hot(self.logits.detach() - torch.log(-torch.log(u))) + (probs - probs.detach())

    def sample(self, deterministic: Union[bool, Tensor], noise: Optional[Tensor] = None) -> Tensor:
        if isinstance(deterministic, Tensor):
            d = deterministic.unsqueeze(-1)
            det, rnd = self._one_hot(self.probs).flatten(-2, -1), self._rnd(noise).flatten(-2, -1)
            return det.masked_fill(~d, 0) + rnd.masked_fill(d, 0)
        return (self._one_hot(self.probs) if deterministic else self._rnd(noise)).flatten(-2, -1)

    def repeat_interleave_(self, repeats: int, dim: int) -> None:
        self._set(self.logits.repeat_interleave(repeats, dim))
        if self.valid is not None:
            self.valid = self.valid.repeat_interleave(repeats, dim)


class DestCategorical(MyDist):
    def __init__(self, probs: Optional[Tensor] = None, logits: Optional[Tensor] = None, valid: Optional[Tensor] = None):
        self.distribution = (Categorical(logits=logits, validate_args=False) if probs is None
                             else Categorical(probs=probs, validate_args=False))
        self.probs, self.valid = self.distribution.probs, valid

    def log_prob(self, sample: Tensor) -> Tensor:
        return self.distribution.log_prob(sample)

    def sample(self, deterministic: Union[bool, Tensor]) -> Tensor:
        if isinstance(deterministic, Tensor):
            return self.probs.argmax(-1).masked_fill(~deterministic, 0) + self.distribution.sample().masked_fill(deterministic, 0)
        return self.probs.argmax(-1) if deterministic else self.distribution.sample()

    def repeat_interleave_(self, repeats: int, dim: int) -> None:
        self.probs = self.probs.repeat_interleave(repeats, dim)
        self.distribution = Categorical(probs=self.probs, validate_args=False)
        if self.valid is not None:
            self.valid = self.valid.repeat_interleave(repeats, dim)
