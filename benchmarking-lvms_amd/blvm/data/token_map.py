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
