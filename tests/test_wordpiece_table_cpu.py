"""The device tokeniser's table (spmm_amd/wordpiece_device.py) without a GPU: `WordPieceTable.tokenize_host` walks the very words the
kernel stages in LDS, with the kernel's per-position algorithm, and must give what `tokenizer.encode_smiles` gives -- on the golden strings
(and through them the Hugging Face ids), on hand-picked edges, on seeded random strings and on made-up vocabularies."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spmm_amd import wordpiece_device as W                         # noqa: E402
from spmm_amd.tokenizer import MAX_LENGTH, SmilesWordPiece, encode_smiles      # noqa: E402

SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab300.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def tok(golden):
    return SmilesWordPiece([str(v) for v in golden["vocab"]])


@pytest.fixture(scope="module")
def table(tok):
    return W.WordPieceTable.from_tokenizer(tok)


def host_rows(table, tok, strings, max_length=MAX_LENGTH):
    """encode_smiles through the table: the strings with a byte the kernel leaves to the host go through the tokenizer, as the wrapper does."""
    rows, status = [], []
    for s in strings:
        row, st = table.tokenize_host(W.word_of(s), max_length - 2)
        rows.append(encode_smiles(tok, [s], max_length)[0] if st == W.STATUS_HOST else row)
        status.append(st)
    return rows, status


def alphabet(tok):
    return sorted({c for p in tok.itos if p not in SPECIALS for c in (p[2:] if p.startswith("##") else p)})


def string_of_pieces(tok, n: int, seed: int = 0) -> str:
    """A string the tokenizer cuts into exactly n pieces (behind '[CLS]'): characters appended one by one, each kept only if it adds a piece."""
    rng = np.random.default_rng(seed)
    alpha, s = alphabet(tok), ""
    count = lambda t: len(tok.tokenize("[CLS]" + t))                   # noqa: E731
    while count(s) < n + 1:
        c = alpha[int(rng.integers(0, len(alpha)))]
        if count(s + c) == count(s) + 1 and tok.tokenize("[CLS]" + s + c)[0] != "[UNK]":
            s += c
    return s


def test_the_table_describes_itself(table, tok):
    w = table.words
    assert w.dtype == np.int32 and w[0] == W.MAGIC and w.size == 4 + w[1] + w[2] <= W.TABLE_MAX
    assert w[2] & (w[2] - 1) == 0 and w[3] == max(len(p) for p in tok.itos) <= W.PIECE_MAX
    used = w[4 + w[1]:] >= 0
    assert used.sum() == w[1] - 2 and used.sum() * 2 <= w[2]          # one edge into every node but the two roots; load <= 1/2
    assert (table.unk_id, table.sep_id, table.pad_id, table.max_chars) == (tok.unk_token_id, tok.sep_token_id, tok.pad_token_id, 250)


def test_golden_strings_and_the_hugging_face_ids(golden, tok, table):
    strings = [str(s) for s in golden["smiles"]]
    rows, status = host_rows(table, tok, strings)
    assert rows == encode_smiles(tok, strings)
    hf, am = golden["input_ids"][:, 1:], golden["attention_mask"][:, 1:]
    for r, ids, m in zip(rows, hf, am):
        assert r == ids[:int(m.sum())].tolist()
    assert sum(s == W.STATUS_HOST for s in status) == sum(any(not 0x21 <= b <= 0x7E for b in s.encode()) for s in strings)


EDGES = ["", "C", "[CLS]", "[CLS", "[CLS]CCO", "[CLS][CLS]", "##C", "#", "C" * 244, "C" * 245, "C" * 246, "[CLS]" + "C" * 245, "[CLS]" + "C" * 246,
         "C" * 300, "CC~CC", "~", "C" * 120 + "~", "c1ccccc1", "CC O", "CC\tO", "CéC", " ", "CCO ", "[PAD]", "[SEP]", "[UNK]"]


def test_edge_strings(tok, table):
    rows, status = host_rows(table, tok, EDGES)
    assert rows == encode_smiles(tok, EDGES)
    by = dict(zip(EDGES, status))
    assert by[""] == by["C" * 245] == by["[CLS]" + "C" * 245] == W.STATUS_OK and by["C" * 246] == by["[CLS]" + "C" * 246] == by["CC~CC"] == W.STATUS_UNK
    assert by["CC O"] == by["CC\tO"] == by["CéC"] == by[" "] == W.STATUS_HOST
    assert rows[0] == [tok.cls_token_id, tok.sep_token_id]


def test_random_strings(tok, table):
    rng = np.random.default_rng(20240)
    alpha = alphabet(tok) + ["~", "!", "`"]                            # (three characters no piece holds)
    assert all(not any(c in p for p in tok.itos) for c in "~!`")
    strings = ["".join(alpha[j] for j in rng.integers(0, len(alpha) - (3 if k % 2 else 0), int(rng.integers(0, 261)))) for k in range(2400)]
    rows, status = host_rows(table, tok, strings)
    ref = encode_smiles(tok, strings)
    assert rows == ref
    assert W.STATUS_HOST not in status                                 # printable ASCII: the table alone decides
    n_unk = sum(r == [tok.unk_token_id, tok.sep_token_id] for r in ref)
    assert 200 < n_unk < 2200 and max(len(r) for r in ref) == MAX_LENGTH - 1      # both outcomes and the truncation occur


def test_truncation_follows_the_word_to_its_end(tok, table):
    """Python tokenises the whole word before it cuts: an unmatched character behind the 98th piece still makes the row [UNK] [SEP]."""
    s = string_of_pieces(tok, 150)
    cuts = [string_of_pieces(tok, n) for n in (96, 97, 98, 99)]           # rows of 97, 98, 99 and 100 entries before the cut
    assert [len(encode_smiles(tok, [c], 1000)[0]) for c in cuts + [s]] == [98, 99, 100, 101, 152]
    for strings in ([s, s + "~"], cuts, [c + "~" for c in cuts]):
        rows, _ = host_rows(table, tok, strings)
        assert rows == encode_smiles(tok, strings)
    assert all(r == [tok.unk_token_id, tok.sep_token_id] for r in host_rows(table, tok, [c + "~" for c in cuts])[0])
    assert host_rows(table, tok, [s + "~"])[0][0] == [tok.unk_token_id, tok.sep_token_id]
    assert host_rows(table, tok, [s], 152)[0] == encode_smiles(tok, [s], 152)


def made_up(pieces):
    return SmilesWordPiece(SPECIALS + list(pieces))


def test_greedy_dead_end_is_unk():
    """Longest match first, no backtracking: 'abc' takes '##ab' and then finds nothing for 'c' -- never '##a' + '##bc'."""
    tok = made_up(["##ab", "##a", "##bc", "##c1"])
    t = W.WordPieceTable.from_tokenizer(tok)
    for s in ("abc", "abcc1", "aab", "abab", "abc1", "a", "bc"):
        assert t.tokenize_host(W.word_of(s))[0] == encode_smiles(tok, [s])[0], s
    assert t.tokenize_host(W.word_of("abc")) == ([tok.unk_token_id, tok.sep_token_id], W.STATUS_UNK)
    assert t.tokenize_host(W.word_of("abc1"))[0] == [tok.cls_token_id, tok.vocab["##ab"], tok.vocab["##c1"], tok.sep_token_id]


def test_plain_and_continuation_pieces_are_different_ids():
    """'C' matches at position 0 only, '##C' everywhere else -- and, as written, at position 0 of a word that starts with '##C'."""
    tok = made_up(["C", "##C", "CC", "##O"])
    t = W.WordPieceTable.from_tokenizer(tok)
    for head in ("", "x"):                                             # without the '[CLS]' head the plain pieces are reachable
        for s in ("C", "CC", "CCC", "CO", "OC", "##C", "##CC", "##", "#"):
            word = (head + s).encode()
            ref = tok.encode(head + s, MAX_LENGTH)[1:] if head + s else None
            if ref is not None:
                assert t.tokenize_host(word)[0] == ref, (head, s)
    assert t.tokenize_host(b"CCC")[0] == [tok.vocab["CC"], tok.vocab["##C"], tok.sep_token_id]
    assert t.tokenize_host(b"##CC")[0] == [tok.vocab["##C"], tok.vocab["##C"], tok.sep_token_id]


def test_a_piece_at_the_length_cap():
    long_piece = "##" + "Z" * (W.PIECE_MAX - 2)
    tok = made_up([long_piece, "##Z"])
    t = W.WordPieceTable.from_tokenizer(tok)
    assert t.words[3] == W.PIECE_MAX
    for n in (W.PIECE_MAX - 3, W.PIECE_MAX - 2, W.PIECE_MAX - 1, 2 * (W.PIECE_MAX - 2)):
        s = "Z" * n
        assert t.tokenize_host(W.word_of(s))[0] == encode_smiles(tok, [s])[0]
    assert t.tokenize_host(W.word_of("Z" * (W.PIECE_MAX - 2)))[0] == [tok.cls_token_id, tok.vocab[long_piece], tok.sep_token_id]


def test_unsupported_vocabularies_are_refused_with_the_reason():
    with pytest.raises(W.WordPieceTableError, match=r"holds a byte outside 0x21\.\.0x7E"):
        W.WordPieceTable.from_tokenizer(made_up(["##C", "##é"]))
    with pytest.raises(W.WordPieceTableError, match=r"holds a byte outside 0x21\.\.0x7E"):
        W.WordPieceTable.from_tokenizer(made_up(["##C O"]))
    with pytest.raises(W.WordPieceTableError, match=rf"is {W.PIECE_MAX + 1} bytes long: the kernel's cap is {W.PIECE_MAX}"):
        W.WordPieceTable.from_tokenizer(made_up(["##" + "Z" * (W.PIECE_MAX - 1)]))
    rng = np.random.default_rng(3)
    letters = [chr(c) for c in range(0x41, 0x5B)]
    big = sorted({"##" + "".join(letters[j] for j in rng.integers(0, 26, 8)) for _ in range(1200)})
    with pytest.raises(W.WordPieceTableError, match=rf"table words: the kernel takes {W.NODES_MAX} nodes and {W.TABLE_MAX} words"):
        W.WordPieceTable.from_tokenizer(made_up(big))
    with pytest.raises(W.WordPieceTableError, match="max_input_chars_per_word=300"):
        W.WordPieceTable.from_tokenizer(SmilesWordPiece(SPECIALS + ["##C"], max_input_chars_per_word=300))


def test_pack_strings_round_trips_and_refuses_newlines():
    strings = ["CCO", "", "c1ccccc1", "Cé", "a b", "", ""]
    blob, offsets = W.pack_strings(strings)
    assert blob.dtype == np.uint8 and offsets.dtype == np.int64 and offsets.shape == (len(strings) + 1,)
    assert W.unpack_strings(blob, offsets) == strings
    assert [bytes(blob[offsets[i]:offsets[i + 1] - 1]) for i in range(len(strings))] == [s.encode() for s in strings]
    for one in ([], [""], ["C"]):
        b, o = W.pack_strings(one)
        assert o.shape == (len(one) + 1,) and W.unpack_strings(b, o) == one
    with pytest.raises(ValueError, match="newline"):
        W.pack_strings(["CC", "C\nC"])
    with pytest.raises(ValueError, match="newline"):
        W.pack_strings(["\n"])


def test_the_module_imports_without_torch():
    import subprocess
    code = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, %r); import spmm_amd.wordpiece_device as W; "
            "print(W.pack_strings(['a', 'b'])[1].tolist())" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "[0, 2, 4]", out.stderr


def test_token_library_from_host_is_todays_batching(tok):
    """TokenLibrary.from_host: the batches of length_sorted_batches + pad_rows, with the host's token count of each."""
    import torch
    from spmm_amd.tokenizer import length_sorted_batches, pad_rows
    strings = ["C" * n for n in (5, 1, 9, 3, 3, 7, 2)] + ["~"]
    rows = encode_smiles(tok, strings)
    lib = W.TokenLibrary.from_host(rows, tok.pad_token_id)
    want = length_sorted_batches([len(r) for r in rows], 3)
    got = list(lib.batches(3))
    assert len(got) == len(want) and len(lib) == len(strings) and not lib.on_device
    for (idx, ids, mask, n_tokens), w in zip(got, want):
        ref_ids, ref_mask = pad_rows([rows[i] for i in w], tok.pad_token_id)
        assert np.array_equal(idx, w) and torch.equal(ids, ref_ids) and torch.equal(mask, ref_mask) and ids.dtype == torch.int64
        assert n_tokens == int(ref_mask.sum())
    ids, mask = lib.padded_host()
    assert torch.equal(ids, pad_rows(rows, tok.pad_token_id)[0]) and torch.equal(mask, pad_rows(rows, tok.pad_token_id)[1])
    lib2 = W.TokenLibrary.from_strings(tok, strings, device="cpu")
    assert lib2.rows == rows and W.device_tokenizer_for(tok, "cpu") is None and W.device_tokenizer_for(tok, "cuda", True) is None
