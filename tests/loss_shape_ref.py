"""A float64 restatement of the training objective's loss shaping (the reference's models/metrics/training.py:90-153: p_loss_for_irrelevant,
w_relevant_agent, temporal_discount) on numpy arrays with axes [rows, agent, step]. No package code, CPU only: what tests/golden/
loss_shape.npz (the reference's own numbers) is reproduced with, and what the kernel (tbx_loss_shape) is compared against.

The one deviation from the reference is the issue's: the agent weight multiplies the reward per (row, agent) over all of its steps (the
reference's `w_mask_rel.unsqueeze(1)` broadcasts only for one agent per row, where the two coincide)."""
import numpy as np

# the order of a setting's row in the fixture's `settings` table
SETTING_FIELDS = ("temporal_discount", "p_loss_for_irrelevant", "loss_for_teacher_forcing", "step_training_start", "w_relevant_agent")
# ... and of its row in `out` (NaN: the reference's compute() left the key out) and `sums` (the metric's raw states)
OUT_KEYS = ("loss", "vae_kl", "diffbar_reward", "dr_il_pos", "dr_il_rot", "dr_il_spd", "dr_rule_apx", "navi_loss", "tl_state_loss")
SUM_KEYS = ("vae_kl", "vae_kl_counter", "diffbar_reward", "diffbar_reward_counter", "navi_loss", "navi_counter", "tl_state_loss", "tl_state_counter")


def discount_chain(tf, discount):
    """m [rows, A, T] float32: m_0 = 1, m_t = tf_t ? 1 : m_{t-1} * discount - float32 products with the discount rounded to float32, the
    reference's chain (training.py:131-134) bit for bit. discount <= 0: ones."""
    tf = np.asarray(tf, dtype=bool)
    m = np.ones(tf.shape, dtype=np.float32)
    if discount > 0:
        g = np.float32(discount)
        for t in range(1, tf.shape[-1]):
            m[..., t] = np.where(tf[..., t], np.float32(1.0), m[..., t - 1] * g)
    return m


def shape(pred_valid, tf, relevant, pick, step_training_start, loss_for_teacher_forcing, p_loss_for_irrelevant, w_relevant_agent,
          temporal_discount, reward=None, reward_valid=None):
    """-> dict: lv, any_valid (bool), w_agent (float32 [rows, A]; ones where any_valid with the weight off), m (float32), and with a reward:
    rv (bool), w (float64: rv ? w_agent * m : 0, the exact product of the two float32 factors), total = sum reward * w (float64), abs_total =
    sum |reward * w|, count = #rv. pick [rows, A] bool: the Bernoulli draw, read only for 0 < p < 1."""
    pv, tf = np.asarray(pred_valid, dtype=bool), np.asarray(tf, dtype=bool)
    T = pv.shape[-1]
    lv = pv.copy()
    if p_loss_for_irrelevant < 1.0:
        keep = np.asarray(relevant, dtype=bool).copy()
        if p_loss_for_irrelevant > 0.0:
            keep |= np.asarray(pick, dtype=bool)
        lv &= keep[..., None]
    lv[..., : min(step_training_start, T)] = False
    if not loss_for_teacher_forcing:
        lv &= ~tf
    any_valid = lv.any(-1)
    w_agent = any_valid.astype(np.float32)
    if w_relevant_agent > 0:
        w_agent = w_agent + np.asarray(relevant, dtype=bool).astype(np.float32) * np.float32(w_relevant_agent)
    m = discount_chain(tf, temporal_discount)
    out = dict(lv=lv, any_valid=any_valid, w_agent=w_agent, m=m)
    if reward is not None:
        rv = lv & np.asarray(reward_valid, dtype=bool)
        w = np.where(rv, w_agent[..., None].astype(np.float64) * m.astype(np.float64), 0.0)
        s = np.asarray(reward, dtype=np.float64) * w
        out.update(rv=rv, w=w, total=float(s.sum()), abs_total=float(np.abs(s).sum()), count=int(rv.sum()))
    return out


def agent_term(err, valid, sh, weighted):
    """A per-agent term (KL, navigation): (sum of err * w_agent over valid & any_valid, sum of |.|, the unweighted count)."""
    v = np.asarray(valid, dtype=bool) & sh["any_valid"]
    e = np.asarray(err, dtype=np.float64) * (sh["w_agent"].astype(np.float64) if weighted else 1.0)
    e = np.where(v, e, 0.0)
    return float(e.sum()), float(np.abs(e).sum()), int(v.sum())
