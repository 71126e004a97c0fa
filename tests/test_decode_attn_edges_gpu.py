"""Every launch path of the single-query decode attention (spmm_amd/csrc/decode.hip: the 24 instantiations of the grouped kernel
decode_attn_mfma_kernel<G, ALLSAME, VARLEN>, the one-wave-per-row kernel decode_attn_kernel with cache_write_kernel) at the smallest shapes
at which the path exists, against the float64 reference of tests/decode_attn_reference.py:

    |got - ref64| <= 2^-8 (A + |ref64|) (1 + 2^-7) + max(8 E32, 4 ulp)       element by element

(bf16 probabilities in front of V, a bf16 output, fp32 everything else: derived in the reference module, nothing taken from what a kernel
gives; the `[tol]` line each check prints is the record of the measured error).  The case lists, and the reason these checks cannot pass
a kernel that drops, doubles or mis-attributes ONE key, are in the reference module and tests/test_decode_attn_reference_cpu.py.

ops.decode_attn / ops.decode_xattn are called on the module's buffers and the whole padded buffers are copied back.  Around every launch:
  * the key / value buffer holds NaN in every cell the reference does not read -- positions past the valid ones, cache rows no ancestry
    entry names at that position, padding columns, rows between packed sources, the cells the launch itself fills from knew / vnew -- and
    ancestry entries past the end name a row that is NaN throughout: out must come out finite;
  * out is a view of a wider, taller buffer full of a sentinel which must keep its bits; the key / value buffer afterwards equals its input
    bit for bit, plus exactly the G x nH new 128-byte rows at (rowmap[r], L - 1) with knew / vnew;
  * every case runs twice into fresh buffers and the results are torch.equal: a missed wait of the LDS-DMA ring shows as a flicker;
  * key-identity cases pin (beam, position) -> cache row -> output row: the output must BE one stored value row.

Measured on an MI355X, the case of each family with the least margin (margin = the largest err / allow over the elements; full listing:
profiles/decode_attn_edges_tol.txt; all 217 cases bit-identical across their two runs, the file takes 3 s):
  a. instantiations        varlen-G7-m3h2-L37of37-fused-len37.20.33   E32=2.195e-07 kernel=3.883e-03 margin=0.516
  b. parting               anc-G3-m2h2-L40of43-s39                    E32=2.157e-07 kernel=2.261e-03 margin=0.474
  c. virtual key counts    anc-G4-m2h2-L11of14-s9                     E32=1.788e-07 kernel=3.908e-03 margin=0.588
  d. cache lengths         anc-G3-m2h2-L63of63-s60                    E32=1.574e-07 kernel=2.217e-03 margin=0.364
  e. t_ptr                 anc-G3-m2h2-L40of48-s38-t44                E32=4.085e-07 kernel=2.332e-03 margin=0.404
  e. knew / vnew           anc-G7-m2h2-L2of4-s0-new                   E32=3.935e-07 kernel=8.197e-03 margin=0.704
  e. knew / vnew, others   anc-G3-m2h2-L19of22-s15-new-rowmap         E32=1.498e-07 kernel=2.389e-03 margin=0.491
  f. shared rows           same-G4-m2h2-L23of26-wide                  E32=2.271e-07 kernel=3.202e-03 margin=0.483
  g. per-row kernel        per_row-G9-m1h2-L9of9-s7                   E32=3.287e-07 kernel=7.454e-03 margin=0.659
  h. variable length       varlen-G4-m3h2-L20of33-fused-len33.5.21    E32=1.713e-07 kernel=4.352e-03 margin=0.619
  i. grid                  same-G2-m3h3-L18of21                       E32=2.069e-07 kernel=3.181e-03 margin=0.504
  j. score extremes        same-G5-m2h2-L40of43-hot_first             E32=1.254e-06 kernel=6.439e-03 margin=0.462
  k. key identity          every case exact (error 0): the output is the stored value row
The margins are those of the CPU model of the walk to three digits.  Two keys sit highest: with so few, a probability near 1/2 is a
whole bf16 rounding step away from its neighbour."""
from types import SimpleNamespace

import pytest
import torch

import decode_attn_reference as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from spmm_amd import ops
    return ops


def run_once(ops, p):
    """One launch of problem p on fresh buffers -> the whole out and key / value buffers, back on the CPU."""
    b, s, H = D.operand_buffers(p), D.launch_spec(p), p.H
    dev = lambda t: None if t is None else t.cuda()
    qkv, kv, out = b.qkv.cuda(), b.kv.cuda(), b.out.cuda()
    q, o = qkv[:, :H], out[:p.R, :H]
    assert (q.stride(0), o.stride(0)) == (p.ldq, p.ldo)
    if p.form == "varlen":
        rows = kv.view(-1, s.tok)
        ops.decode_xattn(q, rows[:, :H], rows[:, H:2 * H], o, nH=p.nH, kv_row0=dev(b.row0), kv_len=dev(b.kv_len), Lkv_max=p.Lkv, kv_seq=dev(b.kv_seq),
                         group=p.G)
    else:
        new = dict(knew=qkv[:, H:2 * H], vnew=qkv[:, 2 * H:3 * H]) if p.new else {}
        ops.decode_attn(q, kv[s.koff:], kv[s.voff:], o, nH=p.nH, Lkv=p.Lkv, seq_stride=s.seq_stride, tok_stride=s.tok, head_stride=s.hs, anc=dev(b.anc),
                        kv_div=s.kv_div, group=p.G, t_ptr=dev(b.t), rowmap=dev(b.rowmap), **new)
    torch.cuda.synchronize()
    return SimpleNamespace(out=out.cpu(), kv=kv.cpu())


def run_case(ops, p):
    """Problem p twice into fresh buffers: the rule of check_output, and both sets of buffers equal bit for bit."""
    got, again = run_once(ops, p), run_once(ops, p)
    D.check_output(p.name, got, p)
    for a, b, what in ((got.out, again.out, "out"), (got.kv, again.kv, "key / value buffer")):
        assert torch.equal(D._bits(a), D._bits(b)), f"{p.name}: two runs differ in {int((D._bits(a) != D._bits(b)).sum())} elements of the {what}"


@pytest.mark.parametrize("p", D.CASES_INSTANTIATIONS, ids=D.case_id)
def test_every_instantiation_of_the_grouped_kernel(ops, p):
    """a. G = 1 .. 8 with shared rows (ALLSAME), with an ancestry table whose beams part six positions before the end, and over a
    variable-length memory (VARLEN: 37, 20 and 33 rows): 3 molecules x 2 heads, 37 keys -- three blocks of shared keys, so the ring of two
    slots wraps; 67 .. 79 virtual keys with the table."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_PARTING, ids=D.case_id)
def test_where_the_ancestries_part(ops, p):
    """b. 40 positions, beams on their own rows from s on: s = 0 (no shared key), 15 / 16 / 17 and 31 / 32 (the block that holds position s
    is wholly shared, mixed, or all per-beam: the wave-uniform `shared block` branch either side of its edge), 39 (only the newest position
    differs) and no difference at all (nv = Lkv).  G = 3 (never launched with a table by the older tests) and G = 5 (the product's)."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_NV, ids=D.case_id)
def test_virtual_key_counts_either_side_of_a_block(ops, p):
    """c. nv = s + G (Lkv - s) at 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, with a table (G = 1 .. 8) and with shared rows: 1, 2, 3 and 4
    blocks -- every value of the ring's `newer` wait, the odd last round, keys past the end re-reading the last one.  nv = 17, 33 and 49
    leave one key in the last block, which the last beam alone sees: an all-masked block for every other beam."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_LKV, ids=D.case_id)
def test_cache_lengths_either_side_of_the_ancestry_loads(ops, p):
    """d. Lkv = 1 and 63 .. 256 with Lmax = Lkv: one to four 64-lane loads of the ancestry table, entries past the end re-reading the
    last, LD = (Lkv + 3) & ~3 with Lkv % 4 = 0, 1, 3; and 256 positions of 8 beams on unrelated rows: 2048 virtual keys, 16 KiB of LDS."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_T_PTR, ids=D.case_id)
def test_device_side_position(ops, p):
    """e. t_ptr with the host's Lkv = Lmax = 256 (a replayed graph) and *t_ptr + 1 at the lengths of d.: positions past *t_ptr hold NaN
    and their table entries name the NaN row; and *t_ptr + 1 = 45 > Lkv = 40, which must clamp."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_NEW, ids=D.case_id)
def test_newest_position_from_the_projection_output(ops, p):
    """e. knew / vnew for every G at Lkv = 1 (nothing but the new key), 2, 17 (two or three blocks, the new keys in the last) and
    256: the cells at (row, Lkv - 1) hold NaN before the launch and the new rows after it; nothing else changes."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_NEW_ARGS, ids=D.case_id)
def test_newest_position_with_t_ptr_rowmap_and_head_major_caches(ops, p):
    """e. knew / vnew under a device-side position (0, 16, 31, and 40 > Lkv - 1: clamped), with a rowmap of scattered, out-of-order rows in
    a cache of 2R + 3 rows (G = 1, 3, 5, 8), in the decoder's head-major cache layout, with head_stride = 72, and all of it together."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_SAME_ARGS, ids=D.case_id)
def test_shared_rows_in_every_layout(ops, p):
    """f. G = 1, 2, 4, 7 (not launched with shared rows by the older tests) over the fused K|V buffer, with seq_stride = 0 (the guided
    search's baseline memory: every molecule reads sequence 0), head_stride = 72 and head-major rows.  23 keys: two blocks."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_PER_ROW, ids=D.case_id)
def test_the_one_wave_per_row_kernel(ops, p):
    """g. decode_attn_kernel through group = 9, 12, 32 with a table -- plain, with knew / vnew (cache_write_kernel), with t_ptr, with both
    (*t_ptr = 18, and 30 > Lkv - 1 = 20: j = min(*t_ptr, Lkv - 1)), with a rowmap into a head-major cache -- and without a table through
    kv_div != group.  Lkv = 1, 7, 8, 9 (the 8-key steps) and 256 (the whole score row); R * nH = 3, 4, 5: a partial, a full and a
    second workgroup of four waves."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_VARLEN, ids=D.case_id)
def test_variable_length_memory(ops, p):
    """h. kv_len = 1, 15, 16, 17, 33 in one launch (per-wave block counts), sources permuted and repeated through kv_seq, lengths above
    Lkv_max (clamped: rows past Lkv_max hold NaN), two NaN rows between the sources and after the last."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_GRID, ids=D.case_id)
def test_grid_rounding_and_xcd_remap(ops, p):
    """i. nmol * nH = 1, 7, 8, 9 waves: a grid rounded up to 8 or 16 workgroups, the remap of blockIdx over the XCDs, idle workgroups."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_EXTREMES, ids=D.case_id)
def test_score_extremes(ops, p):
    """j. All scores equal (identical keys), all zero (queries of zeros), and one key ahead of the rest by more than 100 in the first
    block, the last block and at the first per-beam position: the running-maximum rescale, exp underflow to 0 and an accumulator scaled by
    it; grouped with a table, grouped with shared rows, and per row."""
    run_case(ops, p)


@pytest.mark.parametrize("p", D.CASES_IDENTITY, ids=D.case_id)
def test_key_identity(ops, p):
    """k. Row r's query is 16 x the key of ONE position (weight >= 1 - 2^-30): the output must be that key's stored value row.  The rows
    of a launch sweep every position for every beam: shared prefix, position s, per-beam tail, the newest position from knew / vnew
    through a rowmap, unrelated tables, shared rows, seq_stride = 0, sources found through kv_seq / kv_row0, the per-row kernel."""
    run_case(ops, p)
