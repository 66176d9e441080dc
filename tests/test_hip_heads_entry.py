"""The agents' heads in the step's last launch and their two embedding rows (csrc/dec_layer_mf.inc: lanes 0-31 of wave 0 take the
navigation row, lanes 32-63 the latent row, a quad each). One paired last-layer launch at 16 + 10 rows (agents 2 x 8 with the heads,
lights 2 x 5 with their tail): it writes what its two single launches write, bit for bit, and the heads' actions are those of the
stand-alone heads launch (tbx_heads_tile, csrc/tile_heads.hip - a kernel of its own, which loads the two rows as 16-row tiles) on the
rows the layer stored, bit for bit. On top of the shared case: embeddings that tell the two rows and their 32 quads apart, so that a
swapped select or a wrong quad cannot cancel. Written with the attempt to request these rows ahead of the last linear2 units
(profiles/MEASUREMENT_LOG.md, "Front launch: arguments resolved once": measured and dropped); it holds for any way of loading them."""
import importlib.util
from importlib import import_module
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_dec_layer_tails", Path(__file__).with_name("test_hip_dec_layer_tails.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)
dev, hip, model = T.dev, T.hip, T.model  # (its fixtures)


def test_paired_last_layer_16_10_rows(tb, hip, dev, model):
    """The shared case of tests/test_hip_dec_layer_tails.py at 16 + 10 rows, fp32 tables: paired = single launches, heads = tbx_heads_tile."""
    T.test_every_tail_kind_paired_equals_its_two_single_launches(tb, hip, dev, model, 5, False)


def test_heads_rows_are_told_apart(tb, hip, dev, model):
    """navi_emb[r, c] = 1 + r + c / 256 and latent_emb[r, c] = -(1 + r + c / 256) (every row valid): the paired launch's actions equal
    tbx_heads_tile's on the stored rows, and change when the two tables are swapped."""
    eng = import_module("trafficbots_amd.engine")
    P = import_module("trafficbots_amd.utils.pose_emb")
    pe = P.PoseEmb("pe_xy_yaw", pe_dim=128, theta_xy=1e3).to(dev)
    g = torch.Generator().manual_seed(7)
    na, nb = 16, 10
    sched = eng.DEFAULT.replace(live_rows=1, attn_fold=True, dec_mid=True, dec_layer=True, kv_bf16=False, split_bf16=False, dec_tail_mfma=True)
    ramp = 1.0 + torch.arange(na, device=dev)[:, None] + torch.arange(T.D, device=dev)[None, :] / 256.0
    acts = []
    with eng.use(sched):
        ag = T._Half(tb, hip, eng, dev, 31, 2, 8, 4, 64, 8, False)
        tl = T._Half(tb, hip, eng, dev, 32, 2, 5, 4, 64, 8, False)
        hd, _ = T._heads(hip, model, g, na, dev)
        lt = T._lights(hip, model, g, nb, False, dev)
        hd["navi_valid"].fill_(1), hd["latent_invalid"].fill_(0)
        ag.run(pe, heads=hd), tl.run(pe, lights=lt)  # (single launches once: every weight image is packed outside hip.defer())
        torch.cuda.synchronize()
        for swap in (False, True):
            hd["navi_emb"], hd["latent_emb"] = (-ramp, ramp) if swap else (ramp, -ramp)
            hd["navi_emb"], hd["latent_emb"] = hd["navi_emb"].contiguous(), hd["latent_emb"].contiguous()
            ag.x.copy_(ag.x0), tl.x.copy_(tl.x0), hd["action_out"].fill_(7.0)
            with hip.defer() as ca:
                ag.run(pe, heads=hd)
            with hip.defer() as cl:
                tl.run(pe, lights=lt)
            for a_, l_ in zip(ca, cl):
                hip.launch_dec_layer_pair(a_, l_)
            torch.cuda.synchronize()
            ref = torch.full((na, 2), 7.0, device=dev)
            hip.heads_tile(ag.x.clone(), dict(hd, action_out=ref))
            torch.cuda.synchronize()
            assert float(ref.abs().max()) > 1e-3 and torch.equal(hd["action_out"], ref), (swap, float((hd["action_out"] - ref).abs().max()))
            acts.append(ref)
    assert not torch.equal(acts[0], acts[1])
