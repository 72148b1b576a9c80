"""evaluation.bradley_terry: the MM fit of a cross table, with one virtual drawn game per played pair (host, fp64)."""

import math

import pytest
import torch

from handyrl_amd.evaluation import bradley_terry


def _elo(gamma):
    e = [400.0 * math.log10(g) for g in gamma]
    mean = sum(e) / len(e)
    return [x - mean for x in e]


@pytest.mark.parametrize('w01,w10', [(7.0, 3.0), (0.0, 10.0), (10.0, 0.0), (4.5, 4.5), (123.5, 0.5)])
def test_two_agents_in_closed_form(w01, w10):
    """K = 2: gamma_0 / gamma_1 = (w01 + 0.5) / (w10 + 0.5), so the ratings are +-200 log10 of it."""
    n = w01 + w10
    r = bradley_terry([[0.0, w01], [w10, 0.0]], [[0, n], [n, 0]])
    d = 400.0 * math.log10((w01 + 0.5) / (w10 + 0.5))
    assert r.dtype == torch.float64 and r.shape == (2,)
    assert abs(float(r[0]) - d / 2) <= 1e-9 and abs(float(r[1]) + d / 2) <= 1e-9
    assert abs(float(r.sum())) <= 1e-9


GAMMA = (4.0, 2.0, 1.0, 0.25)


def _table(gamma, n):
    """Exact expected scores: i scores n * gamma_i / (gamma_i + gamma_j) against j."""
    K = len(gamma)
    score = [[0.0 if i == j else n * gamma[i] / (gamma[i] + gamma[j]) for j in range(K)] for i in range(K)]
    games = [[0 if i == j else n for j in range(K)] for i in range(K)]
    return score, games


def test_known_strengths_are_recovered():
    """Expected scores of gamma = (4, 2, 1, 1/4) are the fit's fixed point.  With the prior's share removed (0.5 taken
    from every score and 1 from every count, which the fit adds back) the ratings come back to 1e-6 Elo.  With it the
    error is bounded by the prior's weight: one drawn game in n + 1 per pair moves a pair's expected score by at
    most 0.5 / (n + 1), and d(Elo) / d(score share) = 400 / (ln 10 * s * (1 - s)) <= 400 / (ln 10 * 0.0588 * 0.9412)
    over these pairs' shares (the most lopsided is 1/17 = 0.0588), so with n = 10**6 the shift is below
    0.5e-6 * 3140 = 1.6e-3 Elo; the test asserts 2e-3."""
    n = 10 ** 6
    score, games = _table(GAMMA, n)
    want = _elo(GAMMA)
    bare = bradley_terry([[s - 0.5 if s else 0.0 for s in row] for row in score],
                         [[g - 1 if g else 0 for g in row] for row in games])
    assert max(abs(float(a) - b) for a, b in zip(bare, want)) <= 1e-6
    assert abs(float(bare.mean())) <= 1e-9
    with_prior = bradley_terry(score, games)
    err = max(abs(float(a) - b) for a, b in zip(with_prior, want))
    assert 0.0 < err <= 2e-3
    # the prior pulls towards equality: the spread shrinks
    assert float(with_prior.max() - with_prior.min()) < want[0] - want[3]


def test_permuting_the_agents_permutes_the_ratings():
    score, games = _table(GAMMA, 40)
    score[0][1] += 3.0
    score[1][0] -= 3.0
    base = bradley_terry(score, games)
    perm = [2, 0, 3, 1]
    s = [[score[perm[i]][perm[j]] for j in range(4)] for i in range(4)]
    g = [[games[perm[i]][perm[j]] for j in range(4)] for i in range(4)]
    moved = bradley_terry(s, g)
    for i in range(4):
        assert abs(float(moved[i]) - float(base[perm[i]])) <= 1e-8


def test_an_agent_that_won_everything_stays_finite():
    score = [[0.0, 20.0, 20.0], [0.0, 0.0, 12.0], [0.0, 8.0, 0.0]]
    games = [[0, 20, 20], [20, 0, 20], [20, 20, 0]]
    r = bradley_terry(score, games)
    assert bool(torch.isfinite(r).all()) and float(r[0]) > float(r[1]) > float(r[2])
    assert abs(float(r.sum())) <= 1e-9
    lost = bradley_terry([[0.0, 0.0], [5.0, 0.0]], [[0, 5], [5, 0]])
    assert bool(torch.isfinite(lost).all()) and float(lost[0]) < 0 < float(lost[1])


def test_a_ladder_is_connected_and_two_islands_are_not():
    ladder_games = [[0, 0, 6], [0, 0, 6], [6, 6, 0]]
    ladder_score = [[0.0, 0.0, 2.0], [0.0, 0.0, 3.0], [4.0, 3.0, 0.0]]
    r = bradley_terry(ladder_score, ladder_games)
    assert bool(torch.isfinite(r).all()) and float(r[1]) > float(r[0])
    games = [[0, 6, 0, 0], [6, 0, 0, 0], [0, 0, 0, 6], [0, 0, 6, 0]]
    score = [[0.0, 3.0, 0.0, 0.0], [3.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 4.0], [0.0, 0.0, 2.0, 0.0]]
    with pytest.raises(ValueError, match='connect'):
        bradley_terry(score, games)
    with pytest.raises(ValueError, match='connect'):
        bradley_terry([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [[0, 2, 0], [2, 0, 0], [0, 0, 0]])
