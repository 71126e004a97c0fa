"""The engine's one text pass (Engine.text_rows_of / encode_text, engine.TextRows) without a GPU: when it packs, which tables and
cross-attention sources its consumers get in either layout, and the host layout of pairs gathered from distinct sequences.  Dry-run mode:
every kernel call is validated against the C ABI, none is launched."""
import numpy as np
import pytest
import torch

B, L = 3, 6
LENS = np.array([4, 3, 6], dtype=np.int64)
TP = "text_encoder.bert."


@pytest.fixture
def dry():
    from spmm_amd import ops
    old = ops._DRY_RUN
    ops._DRY_RUN = True
    ops._dry_log.clear()
    yield ops
    ops._DRY_RUN = old


@pytest.fixture
def eng(dry):
    from spmm_amd.config import tiny_config
    from spmm_amd.model import SPMM
    e = SPMM(spmm_config=tiny_config(), no_train=True, device="cpu").eval().engine
    e.train_mode = False
    dry._dry_log.clear()
    return e


def _batch(lens, L_=L):
    mask = (torch.arange(L_)[None, :] < torch.as_tensor(lens)[:, None]).long()
    return (torch.full((len(lens), L_), 5) * mask).to(torch.int32), mask.to(torch.int32), mask


def test_a_padded_batch_with_a_hint_packs_once(dry, eng):
    from spmm_amd.engine import host_token_count
    ids32, mask32, mask = _batch(LENS)
    assert host_token_count(mask) == 13
    t = eng.text_rows_of(TP, eng.cfg.text, ids32, mask32, n_tokens=host_token_count(mask))
    assert dry._dry_log.count("spmm_pack_plan") == 1 and dry._dry_log.count("spmm_gather_rows2") == 1
    assert t.pk is not None and t.pk["M"] == 13 and t.x.shape[0] == 13 and (t.B, t.L) == (B, L) and t.y is None
    assert t.kv_mask is None
    row0, length = t.tables()
    assert row0.data_ptr() == t.pk["row0"].data_ptr() and length.data_ptr() == t.pk["len"].data_ptr()
    g = t.groups.groups[0]
    assert g.causal_from == B and g.nrows == 13 and g.q_row0 is t.pk["row0"] and g.kmask is None
    t.y = t.x
    for src in (t.source(), t.source(tables=True), t.source(proj={"p": None})):
        assert src.row0 is t.pk["row0"] and src.len is t.pk["len"] and src.pack_idx is t.pk["rows"] and (src.U, src.Lkv) == (B, L)
    assert t.source(proj={"p": None}).proj == {"p": None}


def test_a_full_batch_stays_dense(dry, eng):
    ids32, mask32, mask = _batch([L, L, L])
    t = eng.encode_text(TP, eng.cfg.text, ids32, mask32, n_tokens=int(mask.sum()))
    assert "spmm_pack_plan" not in dry._dry_log and "spmm_gather_rows2" not in dry._dry_log
    assert t.pk is None and t.kv_mask is mask32 and t.y.shape == (B * L, eng.cfg.text.hidden_size) and t.tape == [None] * eng.cfg.text.fusion_layer
    row0, length = t.tables()
    assert row0.dtype == length.dtype == torch.int32 and row0.tolist() == [0, 6, 12] and length.tolist() == [6, 6, 6]
    assert t.cls_rows.tolist() == [0, 6, 12] and t.groups.groups[0].kmask is mask32
    plain, tabled = t.source(), t.source(tables=True)
    assert plain.row0 is None and plain.len is None and plain.pack_idx is None and plain.kv is t.y
    assert tabled.row0.tolist() == [0, 6, 12] and tabled.len.tolist() == [6, 6, 6] and tabled.pack_idx is None


def test_causal_and_the_packing_switches(dry, eng):
    ids32, mask32, mask = _batch(LENS)
    assert eng.text_rows_of(TP, eng.cfg.text, ids32, mask32, n_tokens=13, causal=True).groups.groups[0].causal_from == 0
    eng.pack_text = False
    dry._dry_log.clear()
    t = eng.text_rows_of(TP, eng.cfg.text, ids32, mask32, n_tokens=13)
    assert t.pk is None and "spmm_pack_plan" not in dry._dry_log
    assert [x.tolist() for x in t.tables()] == [[0, 6, 12], [4, 3, 6]]            # dense rows, the mask's own lengths


def test_a_length_the_packed_layouts_do_not_hold_never_plans(dry, eng):
    c = eng.cfg.text
    Ll = dry.ATTN_MAXL + 1
    assert Ll <= c.max_position_embeddings
    ids32, mask32, mask = _batch([5, Ll], Ll)
    t = eng.text_rows_of(TP, c, ids32, mask32, n_tokens=int(mask.sum()))
    assert t.pk is None and "spmm_pack_plan" not in dry._dry_log and t.x.shape[0] == 2 * Ll
    ids32, mask32, _ = _batch([5, 9], c.max_position_embeddings + 1)
    dry._dry_log.clear()
    with pytest.raises(ValueError, match=f"^here: sequence length {c.max_position_embeddings + 1} exceeds the {c.max_position_embeddings} position embeddings"):
        eng.text_rows_of(TP, c, ids32, mask32, what="here: ")
    assert dry._dry_log == []                                                    # refused before anything is launched


def test_pair_layout_in_both_layouts(dry, eng):
    ids32, mask32, mask = _batch(LENS)
    inv = np.array([0, 2, 2])
    packed = eng.text_rows_of(TP, eng.cfg.text, ids32, mask32, n_tokens=13)
    lay = packed.pair_layout(LENS, inv)
    assert lay.len_p.tolist() == [4, 6, 6] and lay.qrow0.tolist() == [0, 4, 10] and lay.Mt == 16
    assert lay.gather.tolist() == list(range(0, 4)) + list(range(7, 13)) * 2
    assert lay.pos.tolist() == list(range(4)) + list(range(6)) * 2 and lay.seq.tolist() == [0] * 4 + [1] * 6 + [2] * 6
    eng.pack_text = False
    dense = eng.text_rows_of(TP, eng.cfg.text, ids32, mask32, n_tokens=13)
    lay_d = dense.pair_layout(LENS, inv)
    assert lay_d.gather.tolist() == list(range(0, 4)) + list(range(12, 18)) * 2
    assert all(np.array_equal(a, b) for a, b in zip(lay_d[:5], lay[:5]))         # only the gather index knows the layout


def test_host_prefix_check_has_one_home():
    from spmm_amd import engine, score
    assert score.host_lens is engine.host_lens
    assert engine.host_lens(torch.tensor([[1, 1, 0], [1, 0, 0]]), "t").tolist() == [2, 1]
    for bad in ([[1, 0, 1]], [[0, 1, 1]], [[0, 0, 0]]):
        with pytest.raises(ValueError, match="^t: every attention mask must be a non-empty prefix"):
            engine.host_lens(torch.tensor(bad), "t")
        assert engine.host_token_count(torch.tensor(bad)) is None
    assert engine.host_token_count(torch.tensor([[1, 1, 0], [1, 0, 0]])) == 3
    assert engine.host_token_count(torch.ones(4)) is None and engine.host_token_count([[1, 1]]) is None
    assert engine.host_token_count(torch.zeros(0, 4, dtype=torch.long)) == 0          # no rows: as before, a count and not a refusal
