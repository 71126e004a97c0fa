"""SMILES syntax for constrained PV -> SMILES decoding: a character automaton, its per-token table for the device, and the host reference of
the grammar mask (csrc/syntax.hip, spmm_smiles_mask).  Pure Python + numpy; torch is not needed to import this module.

SYNTAX ONLY.  Checked: parentheses, ring-bond digits, bracket atoms, bond and dot placement, a non-empty molecule.  NOT checked: element
symbols, valence, aromaticity, two-digit ring labels (`%nn`: '%' rejects), a ring opened and closed on the same atom (`C11`), '.' inside a
branch; '@', '/', '\\', ':' and '*' are not in the grammar and reject.

The automaton.  State (q, depth, rings): q one of START, ATOM, RING, OPEN, CLOSE, BOND_A, BOND_B, DOT, BRK0, BRK (or REJECT), depth >= 0 the
parenthesis depth, rings a 10-bit set of the open ring digits.  Outside a bracket (q not BRK0 / BRK):

    letter A-Za-z   from any                          -> ATOM
    '['             from any                          -> BRK0
    digit d         from ATOM, RING, CLOSE, BOND_A    -> RING     rings ^= 1 << d
    '('             from ATOM, RING, CLOSE            -> OPEN     depth += 1
    ')'             from ATOM, RING, CLOSE, depth>=1  -> CLOSE    depth -= 1
    '-' '=' '#'     from ATOM, RING, CLOSE -> BOND_A; from OPEN -> BOND_B
    '.'             from ATOM, RING, CLOSE            -> DOT
    end ([SEP])     from ATOM, RING, CLOSE with depth == 0 and rings == 0: accept

Inside a bracket: ']' from BRK -> ATOM (from BRK0: REJECT, an empty bracket); letters, digits, '+' and '-' -> BRK (digits are no ring
bonds there).  Everything else, the end inside a bracket included, -> REJECT.

cost(state) = depth + popcount(rings) + (1 if q in START, OPEN, BOND_A, BOND_B, DOT) + (2 if BRK0) + (1 if BRK): a number of further
non-[SEP] tokens that is certainly enough to reach an accepting state, given a vocabulary that holds a one-letter piece, ')' , every single
digit a piece can leave open and ']' (SyntaxTable.from_vocab checks exactly that): each of those pieces lowers the cost by one.

The rule for one row that holds t tokens (history[0] = [CLS]; the next token lands at position t; t_last = the last position the search
can write): a non-[SEP] token v is allowed iff it does not reject from the row's state and cost(state after v) <= t_last - t - 1 (a slot
stays for [SEP]); [SEP] is allowed iff the end rule holds.  A row whose history rejects has nothing allowed.

INVARIANT.  While cost(state) <= t_last - t the allowed set is not empty (cost 0 allows [SEP]; cost > 0 allows one of the single pieces
above, which lowers the cost by one while t grows by one), every allowed non-[SEP] token keeps cost(state') <= t_last - (t + 1), and so
following allowed tokens reaches [SEP] at or before t_last with a well-formed string.

The packed table (SyntaxTable.packed, int32 [V, 4], what the kernel stages in LDS) -- word by word for token v:
    word 0   end state from start states 0 .. 7, four bits each (start state s in bits 4s .. 4s+3)
    word 1   bits 0-3: end state from BRK0 (8), bits 4-7: from BRK (9); the rest 0
    word 2   the counters of a start OUTSIDE a bracket: bits 0-9 ring-toggle mask, bits 10-17 `need` (the depth the token needs at its
             start = minus its lowest prefix depth), bits 18-25 depth delta + 128
    word 3   the same for a start INSIDE a bracket
End states: 0 .. 9 as above, 10 = REJECT, 11 = ACCEPT ([SEP] from ATOM / RING / CLOSE; the caller adds depth == 0 and rings == 0).
[PAD], [UNK] and [CLS] reject from every state."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

START, ATOM, RING, OPEN, CLOSE, BOND_A, BOND_B, DOT, BRK0, BRK, REJECT, ACCEPT = range(12)
N_STATES = 10
Q_NAMES = ("START", "ATOM", "RING", "OPEN", "CLOSE", "BOND_A", "BOND_B", "DOT", "BRK0", "BRK", "REJECT", "ACCEPT")
Q_COST = (1, 0, 0, 1, 0, 1, 1, 1, 2, 1)
MASKED = -1e30                      # SPMM_SYNTAX_MASKED: finite, so guidance u + w (c - u) of two masked entries is the sentinel again
SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]")
_AFTER_ATOM = (ATOM, RING, CLOSE)
_LETTERS = frozenset("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")
_DIGITS = frozenset("0123456789")

State = Tuple[int, int, int]        # (q, depth, rings)
INITIAL: State = (START, 0, 0)
REJECTED: State = (REJECT, 0, 0)


def step_char(state: State, ch: str) -> State:
    """One character of the automaton."""
    q, depth, rings = state
    if q >= REJECT:
        return REJECTED
    if q in (BRK0, BRK):
        if ch == "]":
            return (ATOM, depth, rings) if q == BRK else REJECTED
        if ch in _LETTERS or ch in _DIGITS or ch in "+-":
            return (BRK, depth, rings)
        return REJECTED
    if ch in _LETTERS:
        return (ATOM, depth, rings)
    if ch == "[":
        return (BRK0, depth, rings)
    if ch in _DIGITS:
        return (RING, depth, rings ^ (1 << int(ch))) if q in (ATOM, RING, CLOSE, BOND_A) else REJECTED
    if ch == "(":
        return (OPEN, depth + 1, rings) if q in _AFTER_ATOM else REJECTED
    if ch == ")":
        return (CLOSE, depth - 1, rings) if q in _AFTER_ATOM and depth >= 1 else REJECTED
    if ch in "-=#":
        return (BOND_A, depth, rings) if q in _AFTER_ATOM else ((BOND_B, depth, rings) if q == OPEN else REJECTED)
    if ch == ".":
        return (DOT, depth, rings) if q in _AFTER_ATOM else REJECTED
    return REJECTED


def run(text: str, state: State = INITIAL) -> State:
    for ch in text:
        state = step_char(state, ch)
        if state[0] == REJECT:
            return REJECTED
    return state


def accepts(state: State) -> bool:
    """The end rule."""
    return state[0] in _AFTER_ATOM and state[1] == 0 and state[2] == 0


def well_formed(smiles: str) -> bool:
    return accepts(run(smiles))


def cost(state: State) -> int:
    q, depth, rings = state
    if q >= REJECT:
        raise ValueError("cost of a rejected state")
    return depth + bin(rings).count("1") + Q_COST[q]


def _strip(piece: str) -> str:
    return piece[2:] if piece.startswith("##") else piece


def _counters(text: str, inside: bool) -> Tuple[int, int, int]:
    """(depth delta, depth needed at the start, ring-toggle mask) of a piece started inside / outside a bracket -- the bracket class is
    all of the state these three depend on, as long as the piece does not reject."""
    depth = low = mask = 0
    for ch in text:
        if inside:
            inside = ch != "]"
        elif ch == "[":
            inside = True
        elif ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
            low = min(low, depth)
        elif ch in _DIGITS:
            mask ^= 1 << int(ch)
    return depth, -low, mask


class SyntaxTable:
    """The automaton per vocabulary piece.  pieces: the vocabulary as the tokenizer holds it; text[v]: the characters of piece v ('##'
    stripped; None for a special); end[v, s]: end state from start state s; delta / need / toggle [v, c]: the counters for a start outside
    (c = 0) / inside (c = 1) a bracket; packed: int32 [V, 4] (layout in the module's docstring)."""

    def __init__(self, pieces: Sequence[str]):
        self.pieces: List[str] = [str(p) for p in pieces]
        V = self.V = len(self.pieces)
        for s in SPECIALS:
            if s not in self.pieces:
                raise ValueError(f"vocabulary lacks {s}")
        self.sep_id, self.cls_id = self.pieces.index("[SEP]"), self.pieces.index("[CLS]")
        self.text: List[str | None] = [None if p in SPECIALS else _strip(p) for p in self.pieces]
        self.end = np.full((V, N_STATES), REJECT, dtype=np.int32)
        self.delta = np.zeros((V, 2), dtype=np.int32)
        self.need = np.zeros((V, 2), dtype=np.int32)
        self.toggle = np.zeros((V, 2), dtype=np.int32)
        for v, text in enumerate(self.text):
            if v == self.sep_id:
                self.end[v, list(_AFTER_ATOM)] = ACCEPT
            if not text:
                continue                                  # (a special, or an empty piece: rejects everywhere)
            for s in range(N_STATES):
                # depth 256: more than any piece can close, so ')' never rejects here for want of depth -- `need` carries that
                self.end[v, s] = run(text, (s, 256, 0))[0]
            for c in (0, 1):
                self.delta[v, c], self.need[v, c], self.toggle[v, c] = _counters(text, bool(c))
        if int(np.abs(self.delta).max(initial=0)) > 127 or int(self.need.max(initial=0)) > 255:
            raise ValueError("a vocabulary piece changes the parenthesis depth by more than the packed table holds")
        self._check_payable()
        e = self.end.astype(np.int64)
        w0 = sum(e[:, s] << (4 * s) for s in range(8))
        w1 = e[:, 8] | (e[:, 9] << 4)
        cnt = self.toggle.astype(np.int64) | (self.need.astype(np.int64) << 10) | ((self.delta.astype(np.int64) + 128) << 18)
        packed = np.stack([w0, w1, cnt[:, 0], cnt[:, 1]], axis=1)
        self.packed = np.ascontiguousarray(packed.astype(np.uint32).view(np.int32))
        self._memo: Dict[Tuple[int, int, int, int], np.ndarray] = {}

    @classmethod
    def from_vocab(cls, pieces: Sequence[str]) -> "SyntaxTable":
        return cls(pieces)

    def _check_payable(self):
        """cost() must be payable one token at a time: ValueError naming the missing single piece."""
        texts = set(t for t in self.text if t)
        live = [v for v, t in enumerate(self.text) if t and bool((self.end[v] != REJECT).any())]
        if not any(len(t) == 1 and t in _LETTERS for t in texts):
            raise ValueError("syntax: the vocabulary holds no one-letter piece (an atom must be writable in one token)")
        if any("(" in self.text[v] for v in live) and ")" not in texts:
            raise ValueError("syntax: a piece can leave a branch open but the vocabulary lacks the single piece ')'")
        for d in range(10):
            if any((int(self.toggle[v, 0]) | int(self.toggle[v, 1])) >> d & 1 for v in live) and str(d) not in texts:
                raise ValueError(f"syntax: a piece can leave ring bond {d} open but the vocabulary lacks the single piece '{d}'")
        if any(bool(np.isin(self.end[v, :8], (BRK0, BRK)).any()) for v in live) and "]" not in texts:
            raise ValueError("syntax: a piece can leave a bracket atom open but the vocabulary lacks the single piece ']'")

    # -- the table fold (what the kernel does) ---------------------------------------------------------------------------
    def step_token(self, state: State, v: int) -> State:
        q, depth, rings = state
        if q >= REJECT or not 0 <= v < self.V:
            return REJECTED
        c = int(q >= BRK0)
        nq = int(self.end[v, q])
        if nq >= REJECT or depth < self.need[v, c]:
            return REJECTED
        return (nq, depth + int(self.delta[v, c]), rings ^ int(self.toggle[v, c]))

    def fold(self, ids: Sequence[int], state: State = INITIAL) -> State:
        for v in ids:
            state = self.step_token(state, int(v))
        return state

    # -- the character automaton over token ids (the reference) ----------------------------------------------------------
    def state_of(self, ids: Sequence[int], state: State = INITIAL) -> State:
        """State after the pieces `ids` (no [CLS] in front), by the character automaton; any special among them rejects."""
        for v in ids:
            text = self.text[int(v)] if 0 <= int(v) < self.V else None
            if not text:
                return REJECTED
            state = run(text, state)
            if state[0] == REJECT:
                return REJECTED
        return state

    def decode(self, ids: Sequence[int]) -> str:
        return "".join(self.text[int(v)] or "" for v in ids)


def allowed(table: SyntaxTable, history_ids: Sequence[int], t_last: int) -> np.ndarray:
    """The host reference of spmm_smiles_mask for one row: history_ids = the t tokens the row holds (history_ids[0] = [CLS], not looked
    at), the next token lands at position t = len(history_ids) -> bool [V], the tokens that may follow.  Plain Python on the character
    automaton (results are remembered per (state, positions left): many beam rows share a state)."""
    t = len(history_ids)
    state = table.state_of(history_ids[1:])
    if state[0] == REJECT:
        return np.zeros(table.V, dtype=bool)
    key = (*state, int(t_last) - t)
    hit = table._memo.get(key)
    if hit is not None:
        return hit.copy()
    out = np.zeros(table.V, dtype=bool)
    budget = int(t_last) - t - 1                          # non-[SEP] tokens that may still follow v
    for v, text in enumerate(table.text):
        if v == table.sep_id:
            out[v] = accepts(state)
        elif text:
            after = run(text, state)
            out[v] = after[0] != REJECT and cost(after) <= budget
    table._memo[key] = out
    return out.copy()


def check_prefix_state(table: SyntaxTable, prefix_ids: Sequence[int], max_steps: int) -> State:
    """The state a prefix ([CLS] piece_1 ..) leaves the automaton in; ValueError if it rejects or cannot be closed in max_steps tokens."""
    state = table.state_of(list(prefix_ids)[1:])
    shown = table.decode(list(prefix_ids)[1:])
    if state[0] == REJECT:
        raise ValueError(f"syntax: the prefix {shown!r} is not the beginning of a well-formed SMILES string")
    if cost(state) > max_steps:
        raise ValueError(f"syntax: the prefix {shown!r} needs {cost(state)} more tokens to close; max_steps={max_steps} leaves room for "
                         f"{max_steps} and [SEP]")
    return state
