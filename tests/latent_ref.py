"""What tests/golden/make_golden_latent.py and the latent-distribution tests share: the configurations of the `latent_encoder` section
by tag, the c1 scene with its two planted agents, and the model / module configuration of a tag. Data and dict handling only."""
import copy
import zlib

import torch

N_CAT = 8
_D = dict(n_cat=N_CAT, log_std=0.0, mlp_use_layernorm=False, n_layer=3, branch_type=False)
# tag -> overrides of the default latent_encoder section (config.default_model_cfg)
TAGS = {
    "prior_gaus": dict(latent_prior=dict(_D, dist_type="diag_gaus")),
    "branch_std": dict(share_post_prior_encoders=True,
                       latent_post=dict(_D, dist_type="diag_gaus", branch_type=True, log_std=None, mlp_use_layernorm=True),
                       latent_prior=dict(_D, dist_type="diag_gaus", branch_type=True, log_std=None, mlp_use_layernorm=True)),
    "cat_std": dict(latent_post=dict(_D, dist_type="cat"), latent_prior=dict(_D, dist_type="std_cat")),
    "cat_cat": dict(latent_post=dict(_D, dist_type="cat", branch_type=True), latent_prior=dict(_D, dist_type="cat", branch_type=True)),
}
CATEGORICAL = ("cat_std", "cat_cat")
# (tag, p_training_rollout_prior) of the recorded training steps; key in train_c1_latent.npz: f"{tag}_p{p}"
TRAIN_RUNS = [("prior_gaus", 0), ("prior_gaus", 1), ("branch_std", 0), ("cat_cat", 0), ("cat_cat", 1)]
C1 = (1, 8, 64, 8)  # scenes, agents, polylines, lights
# agent seen in the history only at steps the down-sampling (rate 5: steps 0, 5, 10) skips; agent seen in the future only
AG_BETWEEN, AG_FUTURE, N_HIST = 3, 4, 11
KL_GRID = [(0.0, 0.0), (0.0, 1.0), (0.2, 0.0), (0.2, 1.0)]  # (kl_balance_scale, kl_free_nats)
SPOT_PRIOR_ENC = "latent_encoder.ag_encoder_prior.input_encoder.mlp.fc_layers.0.weight"


def prior_head_spot(tag: str) -> str:
    """First layer of the prior head (of its first branch with branch_type)."""
    c = TAGS[tag]["latent_prior"]
    name = "mlp_logits" if c["dist_type"] == "cat" else "mlp_mean"
    return f"latent_encoder.latent_dist_prior.{name}." + ("0." if c["branch_type"] else "") + "fc_layers.0.weight"


def model_cfg(tb, tag, neutral: bool = True):
    """default_model_cfg at the c1 K-nearest size with the tag's latent_encoder section; neutral: every dropout off."""
    mcfg = tb.config.default_model_cfg(n_tgt_knn=4)
    if neutral:
        mcfg["tf_cfg"]["dropout_p"] = 0.0
        mcfg["mp_encoder"]["pl_encoder"]["mlp_dropout_p"] = 0.0
        mcfg["add_navi_latent"]["mlp_dropout_p"] = 0.0
    if tag is not None:
        for k, v in copy.deepcopy(TAGS[tag]).items():
            mcfg["latent_encoder"][k] = tb.config.to_attr(v)
    return mcfg


@torch.no_grad()
def det_fill(tb, model, seed: int = 0) -> None:
    """utils.det_fill, then the same name-keyed fill for the parameters of the `mlp_log_std` heads: det_fill leaves every name that
    contains "log_std" at its constructor value (the fixed log_std parameters), which for these MLPs is the constructor's random draw."""
    tb.utils.det_fill(model, seed)
    for name, p in sorted(model.named_parameters(), key=lambda kv: kv[0]):
        if ".mlp_log_std." not in name:
            continue
        g = torch.Generator().manual_seed((seed * 1000003 + zlib.crc32(name.encode())) % (2 ** 31))
        if p.dim() >= 2:
            v = torch.randn(p.shape, generator=g) * (1.0 / p.shape[-1] ** 0.5)
        elif name.endswith(".weight"):  # LayerNorm
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
        else:
            v = 0.1 * torch.randn(p.shape, generator=g)
        p.copy_(v.to(p.device, p.dtype))


def plant(batch):
    """A copy of a make_scene batch with the two planted agents (validity bits only)."""
    b = {k: v.clone() for k, v in batch.items()}
    v = b["agent/valid"]
    assert bool(v[0, AG_BETWEEN].all()) and bool(v[0, AG_FUTURE].all()), "the planted agents start from fully observed ones"
    v[0, AG_BETWEEN, 0:N_HIST:5] = False
    v[0, AG_FUTURE, :N_HIST] = False
    return b


def c1_batch(tb, agent_valid=None):
    b = plant(tb.synthetic.make_scene(*C1, seed=0))
    if agent_valid is not None:  # (the fixture's stored bits: the test reads them back)
        assert torch.equal(b["agent/valid"], torch.as_tensor(agent_valid))
    return b


def gumbel_sample(logits: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """The sampling convention of the categorical latent, restated for the generator and the tests: index = argmax(logits - log(-log u)),
    ties to the lowest class; value = one_hot + probs - probs.detach(); -> [.., n_cat * n_class]."""
    score = logits.detach() - torch.log(-torch.log(u))
    idx = (score == score.max(-1, keepdim=True).values).to(torch.uint8).argmax(-1)  # first maximum
    probs = torch.softmax(logits, -1)
    return (torch.nn.functional.one_hot(idx, logits.shape[-1]).to(logits.dtype) + (probs - probs.detach())).flatten(-2, -1)
