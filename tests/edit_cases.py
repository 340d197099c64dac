"""Token maps and random index sequences shared by the edit-distance tests: one map per token kind the unit tables must reproduce the
string metrics for.  Every map has the blank "%" at index 0, and the sequences draw it like any other token."""
import random

from blvm.data.token_map import TokenMap, char_tokenizer, word_tokenizer
from blvm.evaluation.metrics import edit_distance

TOKEN_MAPS = {
    "multi_character": TokenMap(["aa", "b", "ch", "d", "eh", "f", "sil"], add_blank=True),
    "space_token": TokenMap(list("abcde") + [" ", "'"], add_blank=True),  # a character vocabulary
    "inner_spaces": TokenMap(["new york", "a b c", "x", " lead", "trail ", "  ", "x y"], add_blank=True),  # "  ": no word at all
}
TOKENIZERS = (word_tokenizer, char_tokenizer)  # in the order of TokenMap.unit_tables()


def random_rows(tm, lengths, seed):
    """One index sequence per entry of `lengths`, every token of the map equally likely."""
    rng = random.Random(seed)
    return [[rng.randrange(len(tm)) for _ in range(n)] for n in lengths]


def string_counts(tm, refs, hyps, tokenizer):
    """Per row (edits, reference length) by today's string path: decode, join with " ", tokenise, host edit distance."""
    out = []
    for ref, hyp in zip(refs, hyps):
        r, h = tokenizer(tm.decode(ref, " ")), tokenizer(tm.decode(hyp, " "))
        out.append((edit_distance(r, h), len(r)))
    return out
