"""The ASG beam search's float32 restatement (tests/asg_beam_ref.py) against a float64 brute force over all paths at
shapes where the beam is exhaustive, and what the decoder and the net refuse without a device."""
import itertools
from pathlib import Path

import numpy as np
import pytest

from asg_beam_ref import TableScorer, asg_beam_search, written_characters

TOY = Path(__file__).resolve().parent / "golden" / "toy_kenlm"
WEIGHTS = (.8, 0., 2.3)


def exported_scorer(characters, lm, weights=WEIGHTS):
    """the restated scorer over the tables of a host scorer for `characters` (the host decoder must outlive the export only)"""
    from speechless_amd.decoder import CtcBeamSearchDecoder, export_scorer_tables
    host = CtcBeamSearchDecoder(characters, lm, beam_width=1, kenlm_weight=weights[0], word_count_weight=weights[1],
                                valid_word_count_weight=weights[2])
    return TableScorer(export_scorer_tables(host._scorer))


def brute_force(logq, trans, init, characters, oracle_scorer):
    """float64: the best prefix over ALL k^T paths (a prefix's score: its best path + its scorer terms + the end term)"""
    t_n, k = logq.shape
    logq, trans, init = (np.asarray(x, dtype=np.float64) for x in (logq, trans, init))
    acoustic = {}
    for path in itertools.product(range(k), repeat=t_n):
        a = init[path[0]] + logq[0, path[0]]
        for t in range(1, t_n):
            a += trans[path[t - 1], path[t]] + logq[t, path[t]]
        prefix = tuple(g for g, _ in itertools.groupby(path))
        acoustic[prefix] = max(acoustic.get(prefix, -np.inf), a)
    best, best_total = None, -np.inf
    for prefix, a in acoustic.items():
        if oracle_scorer is not None:
            state, last = oracle_scorer.initial(), None
            for j in prefix:
                for c in written_characters(j, last, k):
                    state = oracle_scorer.expand(state, c)
                    a = oracle_scorer.expansion_score(state, a)
                last = j
            a += oracle_scorer.end_expansion_score(oracle_scorer.expand_end(state))
        if a > best_total:
            best, best_total = prefix, a
    return list(best), best_total


@pytest.mark.parametrize("characters,t_n", [("at ", 3), ("a", 5)])
@pytest.mark.parametrize("with_lm", [False, True])
def test_restatement_equals_the_brute_force_where_the_beam_is_exhaustive(characters, t_n, with_lm):
    from oracle.beam_search_oracle import ArpaModel, Scorer
    from speechless_amd.decoder import NGramLanguageModel
    k = len(characters) + 2
    scorer = exported_scorer(list(characters), NGramLanguageModel(TOY / "lm.arpa")) if with_lm else None
    oracle = Scorer(ArpaModel(str(TOY / "lm.arpa")), list(characters), *WEIGHTS) if with_lm else None
    rng = np.random.RandomState(11)
    changed = 0
    for case in range(20):
        logq = (rng.randn(t_n, k) * 2).astype(np.float32)
        trans = rng.uniform(-2, 2, size=(k, k)).astype(np.float32)
        init = rng.uniform(-2, 2, size=k).astype(np.float32)
        got, score, _, _ = asg_beam_search(logq, trans, init, t_n, 128, scorer)
        want, want_score = brute_force(logq, trans, init, characters, oracle)
        assert got == want, (case, got, want)
        assert abs(float(score) - want_score) <= 1e-5 * max(1.0, abs(want_score)), (case, score, want_score)
        changed += got != brute_force(logq, trans, init, characters, None)[0]
    if with_lm and len(characters) > 1:
        assert changed > 0  # the model is not a bystander


def test_restatement_edge_cases():
    k = 4
    logq = np.zeros((3, k), dtype=np.float32)
    trans = np.zeros((k, k), dtype=np.float32)
    init = np.zeros((k,), dtype=np.float32)
    assert asg_beam_search(logq, trans, init, 0, 4)[:2] == ([], np.float32("-inf"))
    assert asg_beam_search(logq, trans, np.full(k, -np.inf, dtype=np.float32), 3, 4)[:2] == ([], np.float32("-inf"))
    # all ties: the order rules alone decide -- the first grapheme stays on top, the beam is its first extensions
    assert asg_beam_search(logq, trans, init, 3, 3)[:2] == ([0], np.float32(0))


def test_decoder_limits_raise_before_any_device_call(tmp_path):
    from speechless_amd.decoder import BeamSearchLimitError, GpuAsgBeamSearchDecoder, NGramLanguageModel
    from speechless_amd.synthetic_lm import write_synthetic_arpa
    alphabet = list("acehost ")
    with pytest.raises(BeamSearchLimitError):
        GpuAsgBeamSearchDecoder([chr(0x100 + i) for i in range(63)])  # 65 graphemes
    with pytest.raises(BeamSearchLimitError):
        GpuAsgBeamSearchDecoder(alphabet, beam_width=129)
    with pytest.raises(BeamSearchLimitError):
        GpuAsgBeamSearchDecoder(alphabet, beam_width=0)
    write_synthetic_arpa(tmp_path / "lm.arpa", alphabet, 50, order=7, grams_per_order=5)
    with pytest.raises(BeamSearchLimitError):
        GpuAsgBeamSearchDecoder(alphabet, NGramLanguageModel(tmp_path / "lm.arpa"))
    assert issubclass(BeamSearchLimitError, ValueError)


def test_net_refuses_a_language_model_on_the_host_under_asg():
    from speechless_amd.net import Wav2Letter
    for kw in (dict(), dict(beam_search_device="host")):
        with pytest.raises(ValueError, match="kenlm_directory"):
            Wav2Letter(128, list("acehost "), criterion="asg", kenlm_directory=TOY, **kw)
    with pytest.raises(ValueError, match="beam_search_device"):
        Wav2Letter(128, list("acehost "), criterion="asg", kenlm_directory=TOY, beam_search_device="tpu")
