"""TokenMap: the token <-> index table of the ASR probe, with the reference's interface (blvm/data/token_map.py:19-108), plus the
two string tokenizers the error rates use (blvm/data/tokenizers.py).  The project ships no phoneme or alphabet list: callers pass
their tokens."""
from typing import Iterable, List, Optional

import torch

BLANK_TOKEN = "%"  # the CTC blank (blvm/data/tokens.py:8)


def word_tokenizer(string: str) -> List[str]:
    """The whitespace-separated words of a string."""
    return string.split()


def char_tokenizer(string: str) -> List[str]:
    """The characters of a string."""
    return list(string)


class UnitTable:
    """token index -> list of integer units, in CSR form (the layout `ops.edit_distance` uploads): token v stands for
    units[offsets[v]:offsets[v + 1]], possibly none; `separator` >= 0 goes between every two consecutive tokens of a sequence (not
    before the first, not after the last), < 0: no separator."""

    def __init__(self, unit_lists: Iterable[Iterable[int]], separator: int = -1):
        self.offsets, self.units = [0], []
        for row in unit_lists:
            self.units.extend(int(u) for u in row)
            self.offsets.append(len(self.units))
        self.separator = int(separator)
        self.max_units = max((b - a for a, b in zip(self.offsets, self.offsets[1:])), default=0)

    def __len__(self):
        return len(self.offsets) - 1


def expand_units(indices: Iterable[int], table: UnitTable) -> List[int]:
    """The unit sequence that `table` makes of a token index sequence: the host twin of the expansion in `ops.edit_distance`."""
    if isinstance(indices, torch.Tensor):
        indices = indices.tolist()
    out = []
    for n, v in enumerate(indices):
        if not 0 <= v < len(table):
            raise ValueError(f"expand_units: token index {v} is outside [0, {len(table)})")
        if n and table.separator >= 0:
            out.append(table.separator)
        out.extend(table.units[table.offsets[v] : table.offsets[v + 1]])
    return out


class TokenMap:
    """tokens are SORTED, then `add_blank` puts the blank at index 0."""

    def __init__(self, tokens: Iterable[str], add_blank: bool = False):
        self.add_blank = add_blank
        table = sorted(tokens)
        if len(set(table)) != len(table):
            raise ValueError("TokenMap: tokens must be unique")
        if add_blank:
            table.insert(0, BLANK_TOKEN)
        self.tokens = table
        self.token2index = {t: i for i, t in enumerate(table)}
        self.index2token = dict(enumerate(table))

    def get_index(self, token: str) -> int:
        return self.token2index[token]

    def get_token(self, index: int) -> str:
        return self.index2token[index]

    def encode(self, tokens: Iterable[str]) -> List[int]:
        return [self.get_index(t) for t in tokens]

    def decode(self, indices: Iterable[int], join_separator: Optional[str] = None):
        if isinstance(indices, torch.Tensor):
            indices = indices.tolist()
        out = [self.index2token[i] for i in indices]
        return out if join_separator is None else join_separator.join(out)

    def decode_batch(self, indices_batch, sl, join_separator: Optional[str] = None):
        """Row n's first sl[n] indices, decoded."""
        if isinstance(indices_batch, torch.Tensor):
            indices_batch = indices_batch.tolist()
        if isinstance(sl, torch.Tensor):
            sl = sl.tolist()
        if len(indices_batch) != len(sl):
            raise ValueError("TokenMap.decode_batch: `indices_batch` is batch-first and needs one length per row")
        return [self.decode(row[:n], join_separator) for row, n in zip(indices_batch, sl)]

    def unit_tables(self):
        """(word table, character table): the two `UnitTable`s under which the edit distance between expanded INDEX sequences equals
        the error-rate metrics' distance between tokenised STRINGS, `word_tokenizer(" ".join(tokens))` and
        `char_tokenizer(" ".join(tokens))`.  The joining space isolates the tokens, so the words of the joined string are the
        tokens' own `split()` words in order (none for a whitespace-only token; word ids are interned over the map, no separator),
        and its characters are the tokens' characters with one " " between consecutive tokens (units `ord(c)`, separator
        `ord(" ")`).  The character side needs non-empty tokens (an empty first, last or only token leaves a space in the joined
        string where the separator rule puts none): a map with an empty token has no tables and this returns None, the caller keeps
        to the strings.  Built once per map."""
        if not hasattr(self, "_unit_tables"):
            if any(t == "" for t in self.tokens):
                self._unit_tables = None
            else:
                ids = {}
                words = [[ids.setdefault(w, len(ids)) for w in t.split()] for t in self.tokens]
                chars = [[ord(c) for c in t] for t in self.tokens]
                self._unit_tables = (UnitTable(words), UnitTable(chars, separator=ord(" ")))
        return self._unit_tables

    def __getitem__(self, index: int) -> str:
        return self.get_token(index)

    def __call__(self, token: str) -> int:
        return self.get_index(token)

    def __iter__(self):
        return iter(self.tokens)

    def __len__(self):
        return len(self.tokens)

    def __repr__(self):
        inner = f"tokens={self.tokens}" if len(self.tokens) < 50 else f"|tokens|={len(self.tokens)}"
        return f"TokenMap({inner})"
