"""Device WordPiece (csrc/tokenize.hip, spmm_wordpiece) against tokenizer.encode_smiles: integer outputs, exact equality.  Every launch
writes into arrays pre-filled with -7, so an entry the kernel leaves out shows.  Printable-ASCII inputs must never be left to the host
(status 2); strings with whitespace or UTF-8 must be, and `encode_smiles_device` then returns the host's rows for them."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spmm_amd import wordpiece_device as W                         # noqa: E402
from spmm_amd.tokenizer import MAX_LENGTH, SmilesWordPiece, encode_smiles      # noqa: E402

pytestmark = pytest.mark.gpu
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"]
FILL = -7


@pytest.fixture(scope="module")
def tok():
    g = np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"), allow_pickle=False)
    return SmilesWordPiece([str(v) for v in g["vocab"]])


def alphabet(tok):
    return sorted({c for p in tok.itos if p not in SPECIALS for c in (p[2:] if p.startswith("##") else p)})


def string_of_pieces(tok, n: int, seed: int = 0) -> str:
    """A string the tokenizer cuts into exactly n pieces (behind '[CLS]'), and every prefix of k characters into k: characters appended one
    by one, each kept only if it adds one piece.  n <= 245: the word must stay within the tokenizer's 250 characters."""
    assert n <= 245
    rng = np.random.default_rng(seed)
    alpha, s = alphabet(tok), ""
    while len(s) < n:
        c = alpha[int(rng.integers(0, len(alpha)))]
        pieces = tok.tokenize("[CLS]" + s + c)
        if pieces[0] != "[UNK]" and len(pieces) == len(s) + 2:
            s += c
    return s


@pytest.fixture(scope="module")
def base(tok):
    return string_of_pieces(tok, 245)


def expected(tok, strings, max_length):
    """(ids [N, max_length - 1], lens, status) of the KERNEL: the reference's rows, all padding where the string is the host's."""
    ref = encode_smiles(tok, strings, max_length)
    ids = np.full((len(strings), max_length - 1), tok.pad_token_id, dtype=np.int32)
    lens, status = np.zeros(len(strings), dtype=np.int32), np.zeros(len(strings), dtype=np.int32)
    for i, (s, r) in enumerate(zip(strings, ref)):
        if any(not 0x21 <= b <= 0x7E for b in s.encode()):
            status[i] = W.STATUS_HOST
            continue
        status[i] = W.STATUS_UNK if r == [tok.unk_token_id, tok.sep_token_id] else W.STATUS_OK
        ids[i, :len(r)], lens[i] = r, len(r)
    return ids, lens, status, ref


def launch(tok, blob, offsets, gap, max_length=MAX_LENGTH, table=None, extra_cols=0):
    from spmm_amd import ops
    table = table or W.WordPieceTable.from_tokenizer(tok)
    words, head = table.on("cuda")
    N = len(offsets) - 1
    ids = torch.full((N, max_length - 1 + extra_cols), FILL, dtype=torch.int32, device="cuda")
    lens, status = torch.full((N,), FILL, dtype=torch.int32, device="cuda"), torch.full((N,), FILL, dtype=torch.int32, device="cuda")
    blob_d = torch.from_numpy(np.ascontiguousarray(blob) if len(blob) else np.zeros(1, dtype=np.uint8)).cuda()
    ops.wordpiece(blob_d, torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).cuda(), words, head, ids, lens, status, gap=gap,
                  max_chars=table.max_chars, max_pieces=max_length - 2, unk_id=table.unk_id, sep_id=table.sep_id, pad_id=table.pad_id)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), lens.cpu().numpy(), status.cpu().numpy()


def check(tok, strings, max_length=MAX_LENGTH, host_ok=False, table=None):
    """One launch over `strings` (newline-joined), compared entry by entry; then the wrapper, which must return the reference's rows."""
    blob, offsets = W.pack_strings(strings)
    ids, lens, status = launch(tok, blob, offsets, 1, max_length, table)
    e_ids, e_lens, e_status, ref = expected(tok, strings, max_length)
    assert np.array_equal(status, e_status), (status.tolist(), e_status.tolist())
    assert np.array_equal(lens, e_lens) and np.array_equal(ids, e_ids)
    assert not (ids == FILL).any()
    assert host_ok or not (status == W.STATUS_HOST).any()              # printable ASCII: the device decides every string
    d_ids, d_lens = W.encode_smiles_device(tok, strings, max_length, "cuda", table=table)
    assert d_ids.dtype == torch.int32 and tuple(d_ids.shape) == (len(strings), max_length - 1) and d_ids.is_cuda
    assert isinstance(d_lens, np.ndarray) and d_lens.dtype == np.int32
    d_ids = d_ids.cpu().numpy()
    assert d_lens.tolist() == [len(r) for r in ref]
    for i, r in enumerate(ref):
        assert d_ids[i, :len(r)].tolist() == r and (d_ids[i, len(r):] == tok.pad_token_id).all()
    return status


def pool(tok, n, seed=1):
    """n mixed strings: short and long, tokenisable and not, over the vocabulary's alphabet plus one character no piece holds."""
    rng = np.random.default_rng(seed)
    alpha = alphabet(tok) + ["~"]
    out = []
    for k in range(n):
        m = int(rng.integers(0, 261)) if k % 3 else int(rng.integers(0, 40))
        out.append("".join(alpha[j] for j in rng.integers(0, len(alpha) - (1 if k % 4 else 0), m)))
    return out


@pytest.mark.parametrize("N", [0, 1, 5, 257])
def test_batch_sizes(tok, N):
    """Not a multiple of the four waves of a workgroup, more than one workgroup, and no string at all."""
    status = check(tok, pool(tok, N, seed=N))
    if N == 257:
        assert (status == W.STATUS_OK).sum() > 60 and (status == W.STATUS_UNK).sum() > 30      # (the pool holds both outcomes)


@pytest.mark.parametrize("size", [5, 64, 65, 512])
def test_made_up_vocabularies(size):
    """Table sizes around the staging stride of the workgroup: vocabularies of `size` entries, pieces of one and two characters."""
    letters = [chr(c) for c in range(0x41, 0x5B)]
    pieces = ["##" + a for a in letters] + ["##" + a + b for a in letters[:22] for b in letters[:22]]
    vocab = SPECIALS + pieces[:size - len(SPECIALS)]
    assert len(vocab) == size
    tk = SmilesWordPiece(vocab)
    rng = np.random.default_rng(size)
    strings = ["".join(letters[j] for j in rng.integers(0, 26 if size > 30 else 3, int(rng.integers(0, 120)))) for _ in range(60)] + ["", "A", "AZ", "AAAA"]
    status = check(tk, strings)
    assert (status == W.STATUS_OK).sum() >= 3


def test_word_lengths_at_the_lane_stride_and_the_cap(tok, base):
    """Words (with the 5 bytes of '[CLS]') of 5, 6, 64, 65, 128, 129, 192, 193, 250 bytes are tokenised, 251 is [UNK]; 300 bytes too."""
    base = base + "C" * 60
    word_lens = [5, 6, 64, 65, 128, 129, 192, 193, 250, 251, 305]
    strings = [base[:n - 5] for n in word_lens]
    assert [len(W.word_of(s)) for s in strings] == word_lens
    status = check(tok, strings, max_length=300)                        # (no cut: every piece of the long words is compared)
    assert status.tolist() == [W.STATUS_OK] * 9 + [W.STATUS_UNK] * 2
    check(tok, strings)
    check(tok, [("CCO" * 100)[:n - 5] for n in word_lens] + [("c1ccccc1" * 40)[:n - 5] for n in word_lens])


def test_truncation_follows_the_word_to_its_end(tok, base):
    pieces = [94, 95, 96, 97, 98, 99, 150, 200]
    strings = [base[:n] for n in pieces]
    rows = encode_smiles(tok, strings, 1000)
    assert [len(r) for r in rows] == [n + 2 for n in pieces]           # rows of 96 .. 101, 152 and 202 entries before the cut
    assert {97, 98, 99}.issubset({len(r) for r in rows}) and max(len(r) for r in rows) > 150
    status = check(tok, strings)
    assert (status == W.STATUS_OK).all()
    assert [len(r) for r in encode_smiles(tok, strings)] == [96, 97, 98, 99, 99, 99, 99, 99]
    # an unmatched character behind the 98th piece (and anywhere else) makes the whole row [UNK] [SEP]: Python tokenises, then cuts
    after = [s + "~" for s in strings] + [s + "~" + "C" for s in strings] + [strings[6][:40] + "~" + strings[6][40:], "~", "~C", "C~"]
    assert all(r == [tok.unk_token_id, tok.sep_token_id] for r in encode_smiles(tok, after))
    status = check(tok, after)
    assert (status == W.STATUS_UNK).all()
    check(tok, strings + after, max_length=150)                         # rxn_predict.MAX_SOURCE: 148 pieces at the most
    check(tok, strings + after, max_length=3)                           # one piece


def test_the_head(tok):
    """Strings that already start with '[CLS]' are taken as they are; '[CLS' is not the head."""
    strings = ["[CLS]CCO", "CCO", "[CLS]", "", "[CLS", "[CLS]" + "C" * 245, "[CLS]" + "C" * 246, "[CLS][CLS]", "[CLS]C[CLS]", "[CL", "[", "[CLS]~"]
    status = check(tok, strings)
    ref = encode_smiles(tok, strings)
    assert ref[0] == ref[1] and ref[2] == ref[3] == [tok.cls_token_id, tok.sep_token_id]
    assert status[5] == W.STATUS_OK and status[6] == W.STATUS_UNK


@pytest.mark.parametrize("gap", [0, 1])
def test_every_alignment_of_the_blob(tok, base, gap):
    """String starts at every offset mod 8, with and without the separator byte; the same string gives the same row wherever it stands."""
    strings = ["CCO", "c1ccccc1C", "", "N", base[:130], "CC(=O)O", "~", "CCN(CC)CC", "O", "CCO"]
    e_ids, e_lens, e_status, _ = expected(tok, strings, MAX_LENGTH)
    for lead in range(8):
        parts, offsets = [b"\x00" * lead], [lead]
        for s in strings:
            parts.append(s.encode() + (b"\n" if gap else b""))
            offsets.append(offsets[-1] + len(s.encode()) + gap)
        blob = np.frombuffer(bytearray(b"".join(parts) + b"\x00" * 8), dtype=np.uint8)
        ids, lens, status = launch(tok, blob, offsets, gap, extra_cols=lead % 3)
        W_ = MAX_LENGTH - 1
        assert np.array_equal(ids[:, :W_], e_ids) and np.array_equal(lens, e_lens) and np.array_equal(status, e_status)
        assert (ids[:, W_:] == tok.pad_token_id).all()                  # every entry of the row's stride is written
        assert np.array_equal(ids[0], ids[9])


def test_the_same_string_at_three_places(tok, base):
    s, t = base[:110], "c1ccccc1" * 9
    strings = [s] + pool(tok, 6, seed=2) + [s, t] + pool(tok, 5, seed=3) + [t, s, t]
    blob, offsets = W.pack_strings(strings)
    ids, lens, status = launch(tok, blob, offsets, 1)
    assert np.array_equal(ids[0], ids[7]) and np.array_equal(ids[0], ids[15]) and lens[0] == lens[7] == lens[15] == MAX_LENGTH - 1
    assert np.array_equal(ids[8], ids[14]) and np.array_equal(ids[8], ids[16])
    check(tok, strings)


def test_strings_left_to_the_host(tok):
    """A space, a tab, UTF-8: status 2 from the kernel (row all padding, length 0); the wrapper writes the host's rows in."""
    strings = ["CCO", "CC O", "CC\tO", "CéC", " ", "C" * 300 + " C", "CCO ", "é", "C\x7fC", "c1ccccc1"]
    status = check(tok, strings, host_ok=True)
    assert status.tolist() == [0, 2, 2, 2, 2, 2, 2, 2, 2, 0]
    ids, lens, st = W.encode_smiles_device(tok, strings, MAX_LENGTH, "cuda", return_status=True)
    assert st.tolist() == status.tolist()
    ref = encode_smiles(tok, strings)
    assert ref[1] != ref[0] and lens.tolist() == [len(r) for r in ref]


def test_chunked_launches_give_the_same_rows(tok):
    strings = pool(tok, 41, seed=9) + ["CC O", ""]
    whole = W.encode_smiles_device(tok, strings, MAX_LENGTH, "cuda")
    for chunk in (1, 64, 700):
        part = W.encode_smiles_device(tok, strings, MAX_LENGTH, "cuda", chunk_bytes=chunk)
        assert torch.equal(part[0], whole[0]) and np.array_equal(part[1], whole[1])


def test_a_table_that_does_not_describe_itself_leaves_everything_to_the_host(tok):
    table = W.WordPieceTable.from_tokenizer(tok)
    broken = W.WordPieceTable(table.words.copy(), table.unk_id, table.sep_id, table.pad_id, table.max_chars)
    broken.words[2] *= 2                                                # more slots than there are words
    blob, offsets = W.pack_strings(["CCO", "", "C" * 300])
    ids, lens, status = launch(tok, blob, offsets, 1, table=broken)
    assert status.tolist() == [2, 2, 2] and lens.tolist() == [0, 0, 0] and (ids == tok.pad_token_id).all()
    d_ids, d_lens = W.encode_smiles_device(tok, ["CCO", "", "C" * 300], MAX_LENGTH, "cuda", table=broken)
    assert d_lens.tolist() == [len(r) for r in encode_smiles(tok, ["CCO", "", "C" * 300])]


def test_token_library_batches_on_the_device(tok):
    """The device holder hands out the host holder's batches: same order, same ids and masks, the host's token counts."""
    strings = pool(tok, 37, seed=4) + ["CC O", "~", ""]
    host = W.TokenLibrary.from_strings(tok, strings)
    dev = W.TokenLibrary.from_strings(tok, strings, device="cuda")
    assert dev.on_device and not host.on_device and len(dev) == len(host) == 40 and dev.host_rows() == host.host_rows()
    for (ia, a_ids, a_mask, a_n), (ib, b_ids, b_mask, b_n) in zip(host.batches(16), dev.batches(16)):
        assert np.array_equal(ia, ib) and a_n == b_n and b_ids.dtype == torch.int32 and b_mask.dtype == torch.int32 and b_ids.is_cuda
        assert torch.equal(a_ids, b_ids.cpu().long()) and torch.equal(a_mask, b_mask.cpu().long())
    (h_ids, h_mask), (d_ids, d_mask) = host.padded_host(), dev.padded_host()
    assert torch.equal(h_ids, d_ids) and torch.equal(h_mask, d_mask) and d_ids.dtype == torch.int64 and not d_ids.is_cuda
