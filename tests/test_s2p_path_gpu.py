"""decode.predict_properties (the engine path of SMILES -> PV: S2PDecoder) against the fp32 oracle running the reference's loop
(decode.smiles_to_pv on oracle.OracleModule), tiny configuration, closed-form weights -- as test_step_gpu.py::test_smiles_to_pv_matches_oracle
builds them.  The oracle's runs are computed once per module and shared.

Tolerances.  12 free-running steps: 5e-2 absolute, the project's tolerance for exactly this comparison.  The teacher-forced step and the
53 free-running steps have no earlier tolerance: DESIGN.md section 5's rule -- 1.5 x the deviation of the path that is already trusted, here
the facade loop `smiles_to_pv` on the same GPU against the same oracle -- gives them: the facade loop's deviations were measured on an MI355X and are fixed as constants below with the
tolerances derived from them (figures in the tests' docstrings and in DESIGN.md section 12).  Each test also prints both paths' deviations
and additionally asserts the engine path within 1.5 x of the facade loop's deviation of the same run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_12 = 5e-2
TOL_DEEP_12 = 1.5 * 5.504e-2             # test_twelve_steps_with_two_fusion_layers: 1.5 x the facade loop's measured deviation
FACADE_TF, TOL_TF = 1.703e-03, 1.5 * 1.703e-03     # teacher-forced step 11: the facade loop's deviation measured on an MI355X; 1.5 x that
FACADE_53, TOL_53 = 9.238e-03, 1.5 * 9.238e-03     # 53 free-running steps, B = 7: the same
RULE = 1.5                               # a new path may be 1.5 x as far from the oracle as the trusted one


def _mk(SPMM, cfg, sd):
    m = SPMM(config=None, spmm_config=cfg)
    m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    return m.eval()


@pytest.fixture(scope="module")
def world(env):
    O, SPMM, tiny_config, *_ = env
    from spmm_amd import decode
    sd = O.closed_form_state_dict(O.tiny_cfg())
    om = O.OracleModule(sd, O.tiny_cfg())
    m = _mk(SPMM, tiny_config(), sd)
    _, ids, mask = O.synthetic_batch(5, 20, seed=3)
    want12 = decode.smiles_to_pv(om, ids, mask, n_props=12)
    return dict(O=O, decode=decode, om=om, m=m, ids=ids, mask=mask, want12=want12)


@pytest.fixture(scope="module")
def batch7(world):
    """B = 7, Lt = 20: molecule 0 fills the batch's length, molecule 1 is a single token."""
    _, ids, mask = world["O"].synthetic_batch(7, 20, seed=5)
    ids[1, 1:] = 0
    mask = (ids != 0).long()
    assert int(mask[0].sum()) == 20 and int(mask[1].sum()) == 1
    want53 = world["decode"].smiles_to_pv(world["om"], ids, mask, n_props=53)
    return ids, mask, want53


def test_twelve_steps_match_the_oracle(world):
    d, m = world["decode"], world["m"]
    want = world["want12"]
    got = d.predict_properties(m, world["ids"].cuda(), world["mask"].cuda(), n_props=12).cpu()
    old = d.smiles_to_pv(m, world["ids"].cuda(), world["mask"].cuda(), n_props=12).cpu()
    print(f"[s2p] 12 steps: engine path {(got - want).abs().max().item():.3e}, facade loop {(old - want).abs().max().item():.3e} from the oracle")
    assert got.shape == want.shape == (5, 12)
    assert (got - want).abs().max().item() < TOL_12, (got - want).abs().max().item()
    assert want.std().item() > 1e-2


def test_twelve_steps_with_two_fusion_layers(env):
    """Three text layers with fusion_layer = 1 and two PV layers: a fusion layer below the top one, so the whole-prefix pass over the
    once-projected cross-attention keys / values runs (the tiny configuration has the last-rows-only layer alone).
    Tolerance: 5e-2 is the project's tolerance for the TINY configuration's 12 steps (values of O(0.3)); this stack is deeper and its
    closed-form weights give values up to 2.0, so that figure does not carry over (the facade loop itself ends 5.504e-2 from the oracle
    here, measured on an MI355X; the engine path 5.504e-2 too -- the same element).  Like every comparison without an earlier tolerance
    this one takes DESIGN.md section 5's rule: 1.5 x the trusted path's deviation = 1.5 x 5.504e-2 = 8.256e-2; and the engine path must
    stay within 1.5 x of the facade loop's deviation of the same run."""
    O, SPMM, tiny_config, *_ = env
    from spmm_amd import decode
    cfg, oc = tiny_config(), O.tiny_cfg()
    cfg.text.num_hidden_layers = oc.text.num_hidden_layers = 3
    cfg.prop.num_hidden_layers = oc.prop.num_hidden_layers = 2
    sd = O.closed_form_state_dict(oc)
    om, m = O.OracleModule(sd, oc), _mk(SPMM, cfg, sd)
    _, ids, mask = O.synthetic_batch(5, 20, seed=3)
    want = decode.smiles_to_pv(om, ids, mask, n_props=12)
    got = decode.predict_properties(m, ids, mask, n_props=12).cpu()          # host mask: the packed batch is sized without a device read
    old = decode.smiles_to_pv(m, ids.cuda(), mask.cuda(), n_props=12).cpu()
    print(f"[s2p] 12 steps, 2 fusion layers: engine path {(got - want).abs().max().item():.3e}, facade loop {(old - want).abs().max().item():.3e}")
    dev_old, dev_new = (old - want).abs().max().item(), (got - want).abs().max().item()
    assert dev_new <= TOL_DEEP_12, (dev_new, TOL_DEEP_12)
    assert dev_new <= RULE * dev_old, (dev_new, dev_old)
    assert want.std().item() > 1e-2


def test_teacher_forced_step(world):
    """Step 11 alone on the oracle's own first 11 values: one pass, no compounding.  Measured on an MI355X: the facade loop's own step 11 (same
    prefix, same text) is 1.703e-03 from the oracle, the engine path 1.703e-03; tolerance 1.5 x 1.703e-03 = 2.555e-03, fixed."""
    d, m, O = world["decode"], world["m"], world["O"]
    ids, mask, want = world["ids"], world["mask"], world["want12"]
    B, H, cfg = 5, m.cfg.text.hidden_size, m.cfg
    vals = want[:, :11].cuda()
    prefix = torch.cat([m.property_cls.detach().float().expand(B, -1, -1), m.property_embed(vals.reshape(B, 11, 1))], dim=1)   # [B, 12, H] fp32
    # the facade loop's step 11
    text = m.text_encoder.bert(ids.cuda(), attention_mask=mask.cuda(), return_dict=True, mode="text").last_hidden_state
    pv = m.property_encoder(inputs_embeds=prefix, return_dict=True).last_hidden_state
    fused = m.text_encoder.bert(encoder_embeds=pv, attention_mask=torch.ones(B, 12, dtype=torch.long, device="cuda"), encoder_hidden_states=text,
                                encoder_attention_mask=mask.cuda(), return_dict=True, is_decoder=True, mode="fusion").last_hidden_state
    old = m.property_mtr_head(fused[:, -1:, :]).reshape(B).cpu()
    # the engine path's step 11
    dec = d.S2PDecoder(m, ids.cuda(), mask.cuda(), 12)
    emb = m.engine.embed_generic("property_encoder.", cfg.prop, prefix.reshape(B * 12, H).contiguous(), B, 12)
    dec.xcache[:, :12] = emb.view(B, 12, H)
    dec.pred[:, :11] = vals
    dec.step(11)
    got = dec.pred.cpu()
    assert torch.equal(got[:, :11], want[:, :11])
    dev_old, dev_new = (old - want[:, 11]).abs().max().item(), (got[:, 11] - want[:, 11]).abs().max().item()
    print(f"[s2p] teacher-forced step 11: facade loop {dev_old:.3e}, engine path {dev_new:.3e} from the oracle (tolerance {RULE * dev_old:.3e})")
    assert dev_old < TOL_12                                   # the yard-stick itself is sane: one pass is within the 12-step tolerance
    assert dev_new <= TOL_TF, (dev_new, TOL_TF)
    assert dev_new <= RULE * dev_old, (dev_new, dev_old)


def test_fifty_three_steps(world, batch7):
    """All 53 properties, B = 7 with a single-token molecule and one of the batch's full length.  Measured on an MI355X: the facade loop ends
    9.238e-03 from the oracle, the engine path 9.238e-03; tolerance 1.5 x 9.238e-03 = 1.386e-02, fixed."""
    d, m = world["decode"], world["m"]
    ids, mask, want = batch7
    got = d.predict_properties(m, ids.cuda(), mask.cuda()).cpu()
    old = d.smiles_to_pv(m, ids.cuda(), mask.cuda()).cpu()
    dev_old, dev_new = (old - want).abs().max().item(), (got - want).abs().max().item()
    print(f"[s2p] 53 steps, B=7: facade loop {dev_old:.3e}, engine path {dev_new:.3e} from the oracle (tolerance {RULE * dev_old:.3e}); "
          f"per molecule {[(round(x, 5)) for x in (got - want).abs().max(1).values.tolist()]}")
    assert torch.isfinite(got).all() and want.std().item() > 1e-2
    assert dev_new <= TOL_53, (dev_new, TOL_53)
    assert dev_new <= RULE * dev_old, (dev_new, dev_old)


def test_output_contract(world):
    d, m = world["decode"], world["m"]
    ids, mask = world["ids"].cuda(), world["mask"].cuda()
    got = d.predict_properties(m, ids, mask, n_props=12)
    assert tuple(got.shape) == (5, 12) and got.dtype == torch.float32 and got.device.type == "cuda"
    assert torch.equal(got, d.predict_properties(m, ids, mask, n_props=12))          # no state carried from call to call
    old = d.smiles_to_pv(m, ids, mask, n_props=12)
    assert tuple(old.shape) == (5, 12) and old.device.type == "cuda"
    assert (old.cpu() - world["want12"]).abs().max().item() < TOL_12                 # the facade loop is what it was
