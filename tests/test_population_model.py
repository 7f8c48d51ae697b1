"""CPU tests of the host statement of self-royale's draw and tally (tests/population_model.py) and of the assignments the GPU tests of the grouped
forward use."""
import numpy as np

import population_model as pm
import rng_spec

SEED = 0x9E3779B97F4A7C15


def test_vector_form_equals_the_scalar_statement():
    ids = np.array([0, 1, 2, 77, 65535, 0xFFFFFFFF, 123456789], np.uint64)
    eps = np.array([0, 1, 5, 0, 300, 0xFFFFFFFF, 2], np.uint64)
    for player in (0, 1):
        for seed in (0, 2026, SEED):
            got = pm.population_words(seed, ids, eps, player)
            want = [pm.population_word(seed, int(i), int(k), player) for i, k in zip(ids, eps)]
            assert got.tolist() == want
    # domain 6, block 0, and the player in bit 12 of the second counter word
    assert rng_spec._ctr(pm.DOMAIN_POPULATION, 0, 0, 0, 1, 9, 4) == (6 << 28, 1 << 12, 9, 4)
    assert pm.population_word(SEED, 5, 0, 0) != pm.population_word(SEED, 5, 0, 1) != pm.population_word(SEED, 5, 1, 1)


def test_each_of_four_members_is_drawn_within_five_sigma():
    N, K = 65536, 4
    sigma = np.sqrt(N * 0.25 * 0.75)
    assert abs(sigma - 110.9) < 0.05
    for player in (0, 1):
        for episode in (0, 3):
            m = pm.members(SEED, np.arange(N), episode, player, K)
            n = np.bincount(m, minlength=K)
            assert n.sum() == N and len(n) == K
            assert (np.abs(n - N / 4) <= 5 * sigma).all(), (player, episode, n)


def test_extreme_words_and_a_team_of_one():
    for K in range(1, 17):
        assert pm.choose(0, K) == 0 and pm.choose(0xFFFFFFFF, K) == K - 1
        for w in (1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE):
            assert 0 <= pm.choose(w, K) < K
    assert all(pm.choose(w, 1) == 0 for w in (0, 1, 0x80000000, 0xFFFFFFFF))
    assert not pm.members(SEED, np.arange(1000), 0, 1, 1).any()
    m = pm.members(SEED, np.arange(1000), 2, 0, 16)
    assert [pm.choose(pm.population_word(SEED, e, 2, 0), 16) for e in range(1000)] == m.tolist()


def test_tally_counts_each_seat_from_its_own_view():
    pop = pm.Population(SEED, 100, 6, (3, 2))
    pop.clear(np.zeros(6, np.int64))
    pop.member[:] = [[0, 0], [1, 1], [2, 0], [0, 1], [1, 5], [2, 1]]
    winner = np.array([0, 1, 2, -1, 0, 1], np.int8)
    mask = np.array([1, 1, 1, 1, 1, 0], np.uint8)
    before = pop.member.copy()
    hist = pop.assign(mask, winner, np.ones(6, np.int64))
    assert np.array_equal(hist, before)
    assert pop.status == pm.S_BAD_MEMBER                     # env 4, seat 1: member 5 of a team of 2
    c = pop.counts
    assert c[0, 0].tolist() == [1, 1, 0, 0] and c[0, 1].tolist() == [2, 1, 0, 1] and c[0, 2].tolist() == [1, 0, 1, 0]
    assert c[1, 0].tolist() == [2, 0, 1, 1] and c[1, 1].tolist() == [1, 1, 0, 0]
    assert np.array_equal(pop.member[5], before[5])          # not in the mask: kept
    for p in range(2):
        assert np.array_equal(pop.member[:5, p], pm.members(SEED, 100 + np.arange(5), 1, p, (3, 2)[p]))


def test_gpu_assignments_cover_every_member_the_empty_member_and_the_group_boundary():
    for K in ((1, 1), (2, 3), (4, 4), (16, 16)):
        for N in (1, 15, 16, 17, 33, 77, 4096):
            used = [set(), set()]
            for kind in pm.ASSIGNMENTS:
                a = pm.assignment(kind, N, K)
                assert a.shape == (N, 2) and a.dtype == np.uint8
                for p in range(2):
                    assert a[:, p].max() < K[p]
                    used[p] |= set(a[:, p].tolist())
            if N >= max(K):
                assert used[0] == set(range(K[0])) and used[1] == set(range(K[1])), (K, N)
            a = pm.assignment("one", N, K)
            assert all(len(set(a[:, p].tolist())) == 1 for p in range(2))
            if max(K) > 1:
                a = pm.assignment("empty", N, K)
                assert any(K[p] > 1 and 0 not in a[:, p] for p in range(2))
            a = pm.assignment("alternating", N, K)
            for p in range(2):
                if K[p] > 1:
                    assert (a[1:, p] != a[:-1, p]).all()
    for K, N in (((4, 4), 77), ((16, 16), 4096), ((2, 3), 33)):
        a = pm.assignment("boundary", N, K)
        n = [np.bincount(a[:, p], minlength=K[p]).tolist() for p in range(2)]
        assert 17 in n[0] + n[1] and 16 in n[0] + n[1], (K, N, n)
