"""Device WordPiece: the token rows of a whole library of SMILES strings in one launch (csrc/tokenize.hip, spmm_wordpiece), for the drivers
that read a file of molecules.  `tokenizer.SmilesWordPiece` stays normative -- the device path returns the ids of `tokenizer.encode_smiles` --
and stays the path of single strings, CPU runs and every string the kernel does not decide (a byte outside 0x21..0x7E: whitespace, control
characters, UTF-8).

  WordPieceTable.from_tokenizer(tok)    the vocabulary as the flat int32 table the kernel stages in LDS; refuses (WordPieceTableError, the
                                        reason named) a vocabulary the kernel cannot hold -- the callers then tokenise on the host
  WordPieceTable.tokenize_host(word)    the kernel's algorithm in Python over the same table words: tests the table without a GPU
  pack_strings(strings)                 -> (blob uint8, offsets int64) through one join
  encode_smiles_device(tok, strings)    -> (ids int32 [N, max_length - 1] on the device, lens int32 [N] on the host)
  TokenLibrary                          ids + lens + pad id of a library, host or device, and its length-sorted batches

This module imports without torch (the table, the host walk and the packing are numpy); the device entry points import it when called."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_LENGTH = 100                       # tokenizer.MAX_LENGTH (that module needs torch to import)
HEAD = "[CLS]"                         # tokenizer.with_cls: every word starts with this text
MAGIC = 0x57500001                     # csrc/tokenize.hip: TOK_MAGIC, TOK_TABLE_MAX, TOK_NODES_MAX, TOK_PIECE_MAX, TOK_CHARS_MAX
TABLE_MAX, NODES_MAX, PIECE_MAX, CHARS_MAX = 8192, 4096, 32, 256
ID_MAX = 1 << 23                       # an id shares a word with the piece's length
HASH_MUL = 0x9E3779B1
CHUNK_BYTES = 1 << 28                  # a library whose bytes exceed this goes to the device in several launches
STATUS_OK, STATUS_UNK, STATUS_HOST = 0, 1, 2


class WordPieceTableError(ValueError):
    """The vocabulary does not fit the device tokeniser; the message says why."""


def _printable(b: bytes) -> bool:
    return all(0x21 <= c <= 0x7E for c in b)


class WordPieceTable:
    """`words` int32: [MAGIC, nodes, slots, longest piece | terminal id per node | hash slots], the layout csrc/tokenize.hip documents.
    Node 0 is the root of position 0 (every vocabulary entry as written), node 1 the root of the later positions (the '##' entries by their
    content).  A hash slot is -1 or (node * 128 + byte) << 12 | child at home (key * HASH_MUL mod 2^32) >> (32 - log2 slots), linear probing."""

    def __init__(self, words: np.ndarray, unk_id: int, sep_id: int, pad_id: int, max_chars: int):
        self.words = np.ascontiguousarray(words, dtype=np.int32)
        self.unk_id, self.sep_id, self.pad_id, self.max_chars = int(unk_id), int(sep_id), int(pad_id), int(max_chars)
        self._dev = {}

    @classmethod
    def from_tokenizer(cls, tok) -> "WordPieceTable":
        if not 1 <= tok.max_chars <= CHARS_MAX:
            raise WordPieceTableError(f"max_input_chars_per_word={tok.max_chars}: the kernel's strips hold words of 1..{CHARS_MAX} characters")
        if len(tok.itos) > ID_MAX:
            raise WordPieceTableError(f"{len(tok.itos)} pieces: ids are limited to {ID_MAX}")
        children, term = {}, [-1, -1]

        def insert(root: int, text: bytes, idx: int):
            node = root
            for c in text:
                nxt = children.get((node, c))
                if nxt is None:
                    nxt = children[(node, c)] = len(term)
                    term.append(-1)
                node = nxt
            term[node] = idx

        for piece, idx in tok.vocab.items():             # (the dict: a piece listed twice has the id of its last line)
            try:
                raw = piece.encode("ascii")
            except UnicodeEncodeError:
                raw = b"\xff"
            if not raw:
                continue                                  # (an empty line of the vocabulary file matches nothing)
            if not _printable(raw):
                raise WordPieceTableError(f"piece {piece!r} (id {idx}) holds a byte outside 0x21..0x7E: the kernel tokenises printable ASCII only")
            if len(raw) > PIECE_MAX:
                raise WordPieceTableError(f"piece {piece!r} (id {idx}) is {len(raw)} bytes long: the kernel's cap is {PIECE_MAX}")
            insert(0, raw, idx)
            if raw.startswith(b"##") and len(raw) > 2:
                insert(1, raw[2:], idx)
        nodes, edges = len(term), len(children)
        slots = 2
        while slots < 2 * edges:
            slots *= 2
        n_words = 4 + nodes + slots
        if nodes > NODES_MAX or n_words > TABLE_MAX:
            raise WordPieceTableError(f"the vocabulary needs {nodes} trie nodes and {n_words} table words: the kernel takes {NODES_MAX} nodes "
                                      f"and {TABLE_MAX} words")
        longest = max((len(p) for p in tok.vocab if p), default=1)
        hshift = 32 - (slots.bit_length() - 1)
        table = np.full(slots, -1, dtype=np.int64)
        for (node, c), child in sorted(children.items()):
            key = node * 128 + c
            h = ((key * HASH_MUL) & 0xFFFFFFFF) >> hshift
            while table[h] >= 0:
                h = (h + 1) & (slots - 1)
            table[h] = (key << 12) | child
        words = np.concatenate([np.array([MAGIC, nodes, slots, longest], dtype=np.int64), np.array(term, dtype=np.int64), table])
        return cls(words.astype(np.int32), tok.unk_token_id, tok.sep_token_id, tok.pad_token_id, tok.max_chars)

    # -- the kernel's algorithm on the host, over the same words --------------------------------------------------------------------
    def _child(self, node: int, byte: int) -> int:
        w = self.words
        nodes, slots = int(w[1]), int(w[2])
        key = node * 128 + byte
        h = ((key * HASH_MUL) & 0xFFFFFFFF) >> (32 - (slots.bit_length() - 1))
        for _ in range(slots):
            e = int(w[4 + nodes + h])
            if e < 0:
                return -1
            if e >> 12 == key:
                return e & 4095
            h = (h + 1) & (slots - 1)
        return -1

    def tokenize_host(self, word_bytes: bytes, max_pieces: int = MAX_LENGTH - 2) -> Tuple[List[int], int]:
        """(row, status) of ONE word given whole (the head already in front), as the kernel decides it: the longest piece at every position
        on its own, then the chain from position 0 to the end of the word, then the cut to max_pieces."""
        w = self.words
        nodes, longest = int(w[1]), int(w[3])
        if any(c < 0x21 or c > 0x7E for c in word_bytes):
            return [], STATUS_HOST
        n = len(word_bytes)
        if n > self.max_chars:
            return [self.unk_id, self.sep_id], STATUS_UNK
        length, ident = [0] * n, [0] * n
        for p in range(n):
            node = 0 if p == 0 else 1
            for j in range(min(longest, n - p)):
                node = self._child(node, word_bytes[p + j])
                if node < 0 or node >= nodes:
                    break
                t = int(w[4 + node])
                if t >= 0:
                    length[p], ident[p] = j + 1, t
        row, p = [], 0
        while p < n:
            if length[p] == 0:
                return [self.unk_id, self.sep_id], STATUS_UNK
            row.append(ident[p])
            p += length[p]
        return row[:max_pieces] + [self.sep_id], STATUS_OK

    def on(self, device):
        """The table's words (and the head's bytes) on `device`, uploaded once."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.words).to(device), torch.from_numpy(np.frombuffer(HEAD.encode(), dtype=np.uint8).copy()).to(device))
        return self._dev[key]


def table_of(tokenizer) -> WordPieceTable:
    """The tokenizer's table, built once per tokenizer object."""
    table = getattr(tokenizer, "_device_table", None)
    if table is None:
        table = WordPieceTable.from_tokenizer(tokenizer)
        try:
            tokenizer._device_table = table
        except AttributeError:
            pass
    return table


def word_of(s: str) -> bytes:
    """The bytes of the word the tokenizer sees for string s (tokenizer.with_cls)."""
    return (s if s.startswith(HEAD) else HEAD + s).encode()


def pack_strings(strings: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (blob uint8, offsets int64 [N + 1]): string i is blob[offsets[i] : offsets[i + 1] - 1) -- the strings joined by newlines, found again
    by one scan.  A string that holds a newline is refused (it would be taken for two)."""
    n = len(strings)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)
    blob = np.frombuffer(bytearray("\n".join(strings).encode()), dtype=np.uint8)      # (bytearray: a writable buffer, which torch.from_numpy wants)
    nl = np.flatnonzero(blob == 10)
    if nl.size != n - 1:
        raise ValueError(f"pack_strings: {nl.size - (n - 1)} newline(s) inside the strings; one string per entry, without '\\n'")
    offsets = np.empty(n + 1, dtype=np.int64)
    offsets[0], offsets[n] = 0, blob.size + 1
    offsets[1:n] = nl + 1
    return blob, offsets


def unpack_strings(blob: np.ndarray, offsets: np.ndarray) -> List[str]:
    raw = blob.tobytes()
    return [raw[offsets[i]:offsets[i + 1] - 1].decode() for i in range(len(offsets) - 1)]


def encode_smiles_device(tokenizer, strings: Sequence[str], max_length: int = MAX_LENGTH, device="cuda", table: Optional[WordPieceTable] = None,
                         chunk_bytes: int = CHUNK_BYTES, return_status: bool = False):
    """tokenizer.encode_smiles + pad_rows on the device -> (ids int32 [N, max_length - 1] on `device`, padded with the pad id; lens int32 [N],
    a host numpy array).  One launch (one per `chunk_bytes` of strings beyond that), one device-to-host copy (lens and status together);
    only the strings the kernel leaves to the host (status 2) go through `tokenizer`, and their rows are written in.  Raises
    WordPieceTableError for a vocabulary the kernel cannot hold and ValueError for max_length < 3 (no room for a piece)."""
    import torch
    from . import ops
    from .tokenizer import encode_smiles
    if max_length < 3:
        raise ValueError(f"encode_smiles_device: max_length={max_length} leaves no room for a piece (needs >= 3)")
    table = table_of(tokenizer) if table is None else table
    device = torch.device(device)
    N, W = len(strings), max_length - 1
    words, head = table.on(device)
    ids = torch.empty(N, W, dtype=torch.int32, device=device)
    meta = torch.empty(2, N, dtype=torch.int32, device=device)              # lens | status
    blob, offsets = pack_strings(strings)
    n0 = 0
    while n0 < N:                                                            # whole strings, at most chunk_bytes of them (or one string)
        n1 = N
        if offsets[N] - offsets[n0] > chunk_bytes:
            n1 = max(n0 + 1, int(np.searchsorted(offsets, offsets[n0] + chunk_bytes, side="right")) - 1)
        b0, b1 = int(offsets[n0]), int(offsets[n1]) - 1                      # (the chunk's bytes without the newline behind its last string)
        part = blob[b0:b1] if b1 > b0 else np.zeros(1, dtype=np.uint8)       # (nothing but empty strings: still a pointer to pass)
        ops.wordpiece(torch.from_numpy(part).to(device), torch.from_numpy(offsets[n0:n1 + 1] - b0).to(device), words, head,
                      ids[n0:n1], meta[0, n0:n1], meta[1, n0:n1], gap=1, max_chars=table.max_chars, max_pieces=max_length - 2,
                      unk_id=table.unk_id, sep_id=table.sep_id, pad_id=table.pad_id)
        n0 = n1
    meta_h = meta.cpu().numpy()                                              # the one copy back
    lens, status = meta_h[0].copy(), meta_h[1]
    left = np.flatnonzero(status == STATUS_HOST)
    if left.size:
        rows = encode_smiles(tokenizer, [strings[i] for i in left], max_length)
        patch = np.full((left.size, W), table.pad_id, dtype=np.int32)
        for k, r in enumerate(rows):
            patch[k, :len(r)] = r
            lens[left[k]] = len(r)
        ids[torch.from_numpy(left).to(device)] = torch.from_numpy(patch).to(device)
    return (ids, lens, status) if return_status else (ids, lens)


class TokenLibrary:
    """The token rows of a library: `ids` [N, W] padded with `pad_id` (int64 on the host, or int32 on the device), `lens` (host numpy [N]).
    `batches` hands them out as the drivers batch a library: in order of token length, each batch cut to its longest row."""

    def __init__(self, ids, lens: np.ndarray, pad_id: int, rows: Optional[Sequence[Sequence[int]]] = None):
        self.ids, self.lens, self.pad_id, self.rows = ids, np.asarray(lens), int(pad_id), rows
        self.on_device = ids is not None and ids.device.type != "cpu"

    def __len__(self):
        return len(self.lens)

    @classmethod
    def from_host(cls, rows: Sequence[Sequence[int]], pad_id: int = 0) -> "TokenLibrary":
        """The rows of tokenizer.encode_smiles as they are: every batch is tokenizer.pad_rows of its rows, ids and mask int64 on the host."""
        return cls(None, np.array([len(r) for r in rows], dtype=np.int64), pad_id, rows=rows)

    @classmethod
    def from_strings(cls, tokenizer, strings: Sequence[str], max_length: int = MAX_LENGTH, device=None) -> "TokenLibrary":
        """device None (or a CPU device): SmilesWordPiece on the host; else the device tokeniser on that device."""
        import torch
        if device is None or torch.device(device).type == "cpu":
            from .tokenizer import encode_smiles
            return cls.from_host(encode_smiles(tokenizer, strings, max_length), tokenizer.pad_token_id)
        ids, lens = encode_smiles_device(tokenizer, strings, max_length, device)
        return cls(ids, lens, tokenizer.pad_token_id)

    def take(self, idx: np.ndarray):
        """(ids [B, L], mask [B, L], n_tokens) of the rows `idx`: L their longest row, n_tokens the host's sum of their lengths (what the
        engine's pack plan is sized by).  Host library: int64 tensors on the host, the mask `ids != pad_id` (tokenizer.pad_rows); device
        library: int32 tensors on the device, the mask from the lengths."""
        import torch
        idx = np.asarray(idx, dtype=np.int64)
        n_tokens = int(self.lens[idx].sum())
        if self.rows is not None:
            from .tokenizer import pad_rows
            return pad_rows([self.rows[i] for i in idx], self.pad_id) + (n_tokens,)
        if not hasattr(self, "_lens_dev"):
            self._lens_dev = torch.from_numpy(self.lens.astype(np.int32)).to(self.ids.device)
        L = max(1, int(self.lens[idx].max()))
        sel = torch.from_numpy(idx).to(self.ids.device)
        ids = self.ids.index_select(0, sel)[:, :L].contiguous()
        mask = (torch.arange(L, dtype=torch.int32, device=ids.device)[None, :] < self._lens_dev.index_select(0, sel)[:, None]).to(torch.int32)
        return ids, mask, n_tokens

    def batches(self, batch_size: int):
        """Yields (index array, ids, mask, n_tokens) -- `take` of every batch of tokenizer.length_sorted_batches: in order of token length."""
        from .tokenizer import length_sorted_batches
        for idx in length_sorted_batches(self.lens, batch_size):
            yield (idx,) + self.take(idx)

    def host_rows(self) -> List[List[int]]:
        """The rows as tokenizer.encode_smiles returns them (lists of ids); ONE copy back for a device library."""
        if self.rows is not None:
            return self.rows
        ids = self.ids.cpu().numpy()
        return [ids[i, :n].tolist() for i, n in enumerate(self.lens)]

    def padded_host(self):
        """(ids, mask) int64 [N, longest row] on the host -- tokenizer.pad_rows of the whole library, in ONE copy for a device library."""
        import torch
        from .tokenizer import pad_rows
        if self.rows is not None:
            return pad_rows(self.rows, self.pad_id)
        L = max(1, int(self.lens.max())) if len(self.lens) else 1
        ids = self.ids[:, :L].cpu().to(torch.int64)
        return ids, (ids != self.pad_id).long()


def library_of(tokenizer, strings: Sequence[str], max_length: int = MAX_LENGTH, model=None, host_tokenizer: bool = False) -> TokenLibrary:
    """The TokenLibrary the drivers batch from: tokenised on `model`'s GPU when `device_tokenizer_for` allows it, else on the host."""
    dev = device_tokenizer_for(tokenizer, getattr(model, "device_", None), host_tokenizer) if model is not None else None
    return TokenLibrary.from_strings(tokenizer, strings, max_length, dev)


def add_tokenizer_flags(parser) -> None:
    """--host_tokenizer of the drivers that read a file of molecules."""
    parser.add_argument("--host_tokenizer", action="store_true",
                        help="tokenise the file's molecules with the Python tokenizer, one string at a time (default on a GPU: one launch of "
                             "spmm_wordpiece; single strings always go through the Python tokenizer)")


def device_tokenizer_for(tokenizer, device, host_tokenizer: bool = False):
    """The device the drivers tokenise a library on, or None for the host path: --host_tokenizer, a model that does not run on a GPU, a
    tokenizer that is no SmilesWordPiece, or a vocabulary that does not fit the kernel (the reason is printed).  Why the device is the
    default: tools/bench_tokenize.py's end-to-end medians (profiles/tokenize_bench.json) -- the index build from strings is 6.3 x faster
    through it at 4 096 strings and 6.5 x at 1 000 000, the score loop 3.7 x at 4 096, with bit-identical outputs."""
    import torch
    from .tokenizer import SmilesWordPiece
    if host_tokenizer or device is None or not isinstance(tokenizer, SmilesWordPiece):
        return None
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        return None
    try:
        table_of(tokenizer)
    except WordPieceTableError as e:
        print(f"device tokenizer not used: {e}")
        return None
    return device
