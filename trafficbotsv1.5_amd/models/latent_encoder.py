"""`LatentEncoder` / `DistEncoder` (models/latent_encoder.py:14-253): the CVAE's two latent distributions per agent. The posterior reads
the down-sampled ground-truth episode (window 19), the prior the down-sampled history (3 of the window's 19 slots, left-padded), each
through its own tl / agent encoders (`share_post_prior_encoders`: through one pair, held under both names).

`DistEncoder` is the head on the agent feature, in the reference's whole constructor space and with its parameter names:

    std_gaus   N(0, 1), no parameters that train (`mean`, `log_std`); the encoders are not run (skip_forward)
    diag_gaus  `mlp_mean`, and `mlp_log_std` (log_std None) or the `log_std` Parameter; with branch_type three MLPs each / a 3-entry
               ParameterList, summed over the agent types under mask_type = ~(ag_type & valid)
    std_cat    uniform over n_class = out_dim / n_cat classes in each of n_cat categoricals (`logits`, frozen); skip_forward
    cat        `mlp_logits` (three with branch_type) -> logits [n, A, n_cat, n_class]

each with or without LayerNorm in the MLPs. Posterior and prior must be of one family (both Gaussian or both categorical): the KL is
between them. In eval mode on the device a head is one row chain (the branches as stacked / block-diagonal stages, the way
`ActionHead.emit` runs its); in train mode and on the CPU it is train_graph.dist_head, the differentiable torch form.
`valid` is `ag_valid.any(-1)` AFTER the down-sampling on the encoder path (latent_encoder.py:97-102,122) and over all steps on the
skip_forward path (:91-94)."""
from copy import deepcopy
from typing import Dict, Optional

import torch
from torch import Tensor, nn

from .. import hip
from ..engine import kv_tables
from ..hip import BUF0, BUF1, Chain
from ..utils.pose_emb import PoseEmb
from .agent_encoder import AgentEncoder
from .modules.distributions import DiagGaussian, MultiCategorical, MyDist
from .modules.mlp import MLP
from .traffic_light import TrafficLightEncoder

FAMILY = {"std_gaus": "gaussian", "diag_gaus": "gaussian", "std_cat": "categorical", "cat": "categorical"}


class DistEncoder(nn.Module):
    def __init__(self, hidden_dim: int, out_dim: int, branch_type: bool, dist_type: str, mlp_use_layernorm: bool,
                 log_std: Optional[float], n_cat: int, n_layer: int) -> None:
        super().__init__()
        if dist_type not in FAMILY:
            raise NotImplementedError(f"DistEncoder: dist_type {dist_type!r}; accepted: {', '.join(FAMILY)}")
        self.dist_type, self.branch_type = dist_type, branch_type
        self.hidden_dim, self.out_dim = hidden_dim, out_dim
        self.skip_forward = dist_type in ("std_gaus", "std_cat")
        head = lambda: MLP([hidden_dim] * n_layer + [out_dim], end_layer_activation=False, use_layernorm=mlp_use_layernorm)
        heads = lambda: nn.ModuleList([head() for _ in range(3)]) if branch_type else head()
        if dist_type == "std_gaus":
            self.mean = nn.Parameter(torch.zeros(1, 1, out_dim), requires_grad=False)
            self.log_std = nn.Parameter(torch.zeros(out_dim), requires_grad=False)
        elif dist_type == "diag_gaus":
            self.mlp_mean = heads()
            if log_std is None:
                self.log_std = None
                self.mlp_log_std = heads()
            elif branch_type:
                self.log_std = nn.ParameterList([nn.Parameter(log_std * torch.ones(out_dim), requires_grad=True) for _ in range(3)])
            else:
                self.log_std = nn.Parameter(log_std * torch.ones(out_dim), requires_grad=True)
        else:
            assert out_dim % n_cat == 0
            self.n_cat, self.n_class = n_cat, out_dim // n_cat
            if dist_type == "std_cat":
                self.logits = nn.Parameter(torch.zeros(1, 1, self.n_cat, self.n_class), requires_grad=False)
            else:
                self.mlp_logits = heads()

    def _branches(self, mlps, x2: Tensor, type_mask: Tensor) -> Tensor:
        """sum over the types i of (type_mask[i] ? 0 : mlps[i](x)) as one row chain: layer 1 of the three MLPs as one stacked stage on
        the shared input, the later layers as block-diagonal stages, LayerNorm per branch, the masked sum in the storing stage."""
        d, G, rows = self.hidden_dim, len(mlps), x2.shape[0]
        layers = [m.linear_layers() for m in mlps]
        n_lin = len(layers[0])
        assert n_lin >= 2 and d % 16 == 0 and self.out_dim <= d
        pad = ((self.out_dim + 15) // 16) * 16
        out = torch.empty(rows, self.out_dim, dtype=torch.float32, device=x2.device)
        ch = Chain(16, G * d + 4)
        ch.load(x2, BUF1, 0, n=d)
        cur, nxt = BUF1, BUF0
        for j in range(n_lin):
            last = j == n_lin - 1
            w, b = hip.stacked_linear([l[j][0] for l in layers], pad_out_to=pad if last else 0)
            ln, act = layers[0][j][1], layers[0][j][2]
            stride = pad if last else d
            if j == 0:
                ch.linear(cur, 0, nxt, 0, w, b, relu=act and ln is None)
            else:
                ch.linear(cur, 0, nxt, 0, w, b, relu=act and ln is None, groups=G, src_stride=d, dst_stride=stride)
            if ln is not None:
                for g in range(G):
                    m = layers[g][j][1]
                    ch.layernorm(nxt, g * stride, nxt, g * stride, m.weight, m.bias, m.eps)
                if act:
                    ch.clamp(nxt, 0, G * stride, 0.0, float("inf"))
            cur, nxt = nxt, cur
        ch.store_masked_sum(cur, 0, self.out_dim, pad, type_mask, out)
        ch.run(rows)
        return out

    def _head(self, mlps, x: Tensor, valid: Tensor, ag_type: Tensor) -> Tensor:
        if not self.branch_type:
            return mlps(x, ~valid)
        tm = (~(ag_type & valid.unsqueeze(-1))).permute(2, 0, 1).reshape(3, -1).to(torch.uint8).contiguous()
        return self._branches(mlps, x.reshape(-1, self.hidden_dim).contiguous().float(), tm).view(*valid.shape, self.out_dim)

    def masked_log_std(self, valid: Tensor, ag_type: Tensor) -> Tensor:
        """The `log_std` list summed over the types with 0 where mask_type is set (latent_encoder.py:231-234) -> [n, A, out_dim]."""
        m = (ag_type & valid.unsqueeze(-1)).unsqueeze(-1).to(self.log_std[0].dtype)
        return (m * torch.stack(list(self.log_std), 0)).sum(2)

    def forward(self, x: Tensor, valid: Tensor, ag_type: Tensor) -> MyDist:
        if self.dist_type == "std_gaus":
            return DiagGaussian(self.mean.expand(*valid.shape, -1), self.log_std, valid=valid)
        if self.dist_type == "std_cat":
            return MultiCategorical(self.logits.expand(*valid.shape, -1, -1), valid=valid)
        if self.dist_type == "diag_gaus" and not self.branch_type and self.log_std is not None:  # the default posterior
            return DiagGaussian(self.mlp_mean(x, ~valid), self.log_std, valid=valid)
        if self.training or not x.is_cuda:
            from .. import train_graph as TG

            x2 = x.reshape(-1, self.hidden_dim).contiguous().float()
            if not self.training:  # (no dropout scope: an eval-mode forward draws nothing from torch's generator)
                return TG.dist_head(self, x2, valid, ag_type)
            with TG.module_scope(1, x.device):
                return TG.dist_head(self, x2, valid, ag_type)
        if self.dist_type == "cat":
            return MultiCategorical(self._head(self.mlp_logits, x, valid, ag_type).view(*valid.shape, self.n_cat, self.n_class), valid=valid)
        mean = self._head(self.mlp_mean, x, valid, ag_type)
        if self.log_std is None:
            log_std = self._head(self.mlp_log_std, x, valid, ag_type)
        else:
            log_std = self.masked_log_std(valid, ag_type) if self.branch_type else self.log_std
        return DiagGaussian(mean, log_std, valid=valid)


class LatentEncoder(nn.Module):
    def __init__(self, latent_dim: int, temporal_down_sample_rate: int, share_post_prior_encoders: bool, latent_prior,
                 latent_post, tl_encoder, ag_encoder, pose_rpe: Optional[PoseEmb], time_step_gt: int):
        super().__init__()
        self.out_dim, self.dummy = latent_dim, latent_dim <= 0
        self.temporal_down_sample_rate = temporal_down_sample_rate
        if self.dummy:
            return
        fam = lambda c: FAMILY.get(c["dist_type"])
        if fam(latent_post) is not None and fam(latent_prior) is not None and fam(latent_post) != fam(latent_prior):
            raise ValueError(f"LatentEncoder: latent_post.dist_type {latent_post['dist_type']!r} ({fam(latent_post)}) and latent_prior.dist_type "
                             f"{latent_prior['dist_type']!r} ({fam(latent_prior)}) are of different families: the KL needs both Gaussian or both categorical")
        r = temporal_down_sample_rate
        win = (time_step_gt + 1) // r + 1 if r > 1 else time_step_gt + 1
        tl_encoder, ag_encoder = deepcopy(tl_encoder), deepcopy(ag_encoder)
        tl_encoder["temp_window_size"] = win
        ag_encoder["temp_window_size"] = win
        self.tl_encoder_post = TrafficLightEncoder(pose_rpe=pose_rpe, **tl_encoder)
        self.ag_encoder_post = AgentEncoder(pose_rpe=pose_rpe, **ag_encoder)
        if share_post_prior_encoders:
            self.tl_encoder_prior, self.ag_encoder_prior = self.tl_encoder_post, self.ag_encoder_post
        else:  # run by a learned prior (diag_gaus / cat); dead weight under std_gaus / std_cat, kept for state-dict parity
            self.tl_encoder_prior = TrafficLightEncoder(pose_rpe=pose_rpe, **tl_encoder)
            self.ag_encoder_prior = AgentEncoder(pose_rpe=pose_rpe, **ag_encoder)
        self.latent_dist_prior = DistEncoder(ag_encoder["hidden_dim"], latent_dim, **latent_prior)
        self.latent_dist_post = DistEncoder(ag_encoder["hidden_dim"], latent_dim, **latent_post)

    @property
    def categorical(self) -> bool:
        return not self.dummy and FAMILY[self.latent_dist_post.dist_type] == "categorical"

    def forward(self, ag_valid: Tensor, ag_attr: Tensor, ag_motion: Tensor, ag_pose: Tensor, ag_type: Tensor,
                tl_state: Tensor, mp_tokens: Dict[str, Tensor], tl_tokens: Dict[str, Tensor], posterior: bool) -> Optional[MyDist]:
        if self.dummy:
            return None
        dist = self.latent_dist_post if posterior else self.latent_dist_prior
        if dist.skip_forward:
            return dist(ag_attr, ag_valid.any(-1), ag_type)
        r = self.temporal_down_sample_rate
        if r > 1:
            assert (ag_valid.shape[-1] - 1) % r == 0
            ag_valid, ag_motion, ag_pose, tl_state = ag_valid[:, :, ::r], ag_motion[:, :, ::r], ag_pose[:, :, ::r], tl_state[:, :, ::r]
        tl_enc = self.tl_encoder_post if posterior else self.tl_encoder_prior
        ag_enc = self.ag_encoder_post if posterior else self.ag_encoder_prior
        n, A, _ = ag_valid.shape
        L = tl_state.shape[1]
        hist_tl = tl_enc.states_to_hist(tl_state, tl_enc.temp_window_size)
        tl_feat = tl_enc.encode(hist_tl, tl_tokens)
        tl_kv = kv_tables(tl_feat, ag_enc.tl_kv_layers())
        hv, hp, hm = ag_enc.pad_hist(ag_valid, ag_pose, ag_motion, ag_enc.temp_window_size)
        feat, _ = ag_enc.encode(hv, hp, hm, ag_attr.float().contiguous(), mp_tokens, tl_tokens["tl_token_invalid_u8"],
                                tl_tokens["tl_token_pose"], tl_kv, mp_batch_div=tl_tokens.get("mp_batch_div", 1))
        return dist(feat.view(n, A, -1), ag_valid.any(-1), ag_type)
