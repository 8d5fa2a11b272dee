"""Seeded random columns and patterns through the host twin of msj_match_strings_device (tests/match_strings_math_host.cpp)
against ``re`` (tests/test_match_strings_math.py: ``py_match``): every generated case is compared, whole outputs, none is
skipped.  Small alphabets, so that pieces repeat, overlap themselves and straddle row borders."""
import random

import pytest

from tests import test_match_strings_math as tmm
from tests.test_match_strings_math import tw  # noqa: F401


@pytest.mark.parametrize("seed", range(6))
def test_random_columns_against_re(tw, seed):  # noqa: F811
    rng = random.Random(1000 + seed)
    c = tmm.constants(tw)
    for _ in range(25):
        alphabet = rng.choice((b"ab", b"abA", b"a\nB", bytes(tmm.ALPHABET)))
        n_rows = rng.choice((0, 1, 5, 40, 300))
        rows = []
        for _ in range(n_rows):
            r = rng.random()
            ln = rng.choice((0, 1, 2, 3, 7, 20, 64))   # (short: ``re`` backtracks over four lazy gaps)
            rows.append(None if r < 0.05 else ("null", tmm.word(rng, ln, alphabet)) if r < 0.1 else tmm.word(rng, ln, alphabet))
        col = tmm.Column(rows, lead=tmm.word(rng, rng.randrange(3), alphabet), tail=tmm.word(rng, rng.randrange(3), alphabet), residue=rng.randrange(16))
        specs = []
        for _ in range(rng.randrange(1, 17)):
            pieces = [tmm.word(rng, rng.choice((1, 1, 2, 2, 3, 5)), alphabet) for _ in range(rng.randrange(1, 5))]
            specs.append((pieces, rng.randrange(8)))
        tmm.check_twin(tw, col, specs, blocks=rng.choice((0, 1, 2)), stage=rng.choice((0, c["chunk"])))
