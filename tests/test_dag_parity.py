"""The exact plan replay (PlanRun(exact_extractions=True): a shared extraction is read from its leader's accumulator, as
the device reads it) and the word-for-word comparison built on it (oracle/dag_parity.py), without a GPU.  The device
half is tests/test_dag_parity_device.py.

  * the exact replay in the f64-FFT mirror (oracle mode 3) decrypts like Python and like the regular expression;
  * negative control: exact and default replay (followers as bootstraps of their own) of one plan decrypt alike and
    differ in words -- which is what lets the device comparison tell "extracted from the leader" from "rotated on its
    own" (f64 arithmetic: the rounding of the FFT differs between the two accumulators; in exact arithmetic they agree
    except at decomposition ties, so nothing is asserted there);
  * the mismatch reporter names result, character, block and word."""
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def small(oracle_keys, oracle_sk):
    """the smallest shape that shares rotations (`zama!\\0` / `ma`: 18 rotations + 4 extractions), exact replay, mode 3"""
    from oracle import dag_parity
    script, string_mode, inputs = dag_parity.case("small", oracle_keys)
    return script, inputs, dag_parity.replay(script, inputs, oracle_sk, 3, string_mode)


def test_exact_replay_of_contains_clear_decrypts_like_python(small, oracle_keys, oracle_sk):
    from oracle import dag_parity
    script, inputs, hit = small
    text = inputs["clear"]
    assert (hit.rotations, hit.extractions, hit.plan["launch_groups"]) == (18, 4, [12, 5, 1])
    assert hit.words["contains_clear"].shape == (1, 4, 2049) and np.array_equal(hit.words["text"], inputs["text"])
    miss = dag_parity.replay(script, dict(inputs, pattern="xy"), oracle_sk, 3)
    for pattern, run in (("ma", hit), ("xy", miss)):
        got = oracle_keys.decrypt_char(run.words["contains_clear"][0])
        assert got == int(pattern.encode() in text) == int(re.search(re.escape(pattern.encode()), text) is not None), pattern
    assert miss.extractions > 0


def test_exact_replay_of_like_clear_decrypts_like_the_regular_expression(oracle_keys, oracle_sk):
    """script C: the one place where two extractions of one rotation are added together"""
    import __graft_entry__
    from oracle import dag_parity
    script, string_mode, inputs = dag_parity.case("C", oracle_keys)
    run = dag_parity.replay(script, inputs, oracle_sk, 3, string_mode)
    text = inputs["clear"]
    assert run.extractions > 0
    body = text.split(b"\0")[0].lower()
    python = {"like": int(any(body[i:i + 1] == b"a" and body[i + 2:i + 3] == b"c" for i in range(len(body) - 2))),
              "like_escaped": int(b"a_c" in body)}
    for name, pattern, escape in (("like", inputs["like"], None), ("like_escaped", inputs["like_escaped"], inputs["escape"])):
        want = __graft_entry__._like_python(text, pattern.encode(), escape.encode() if escape else None, ignore_case=True)
        assert oracle_keys.decrypt_char(run.words[name][0]) == want == python[name] == 1, name
    # ... and on a text without the pattern's `c`
    miss = text.replace(b"c", b"d").replace(b"C", b"D")
    run = dag_parity.replay(script, dict(inputs, text=dag_parity.encrypt(oracle_keys, miss)), oracle_sk, 3, string_mode)
    for name, pattern, escape in (("like", inputs["like"], None), ("like_escaped", inputs["like_escaped"], inputs["escape"])):
        want = __graft_entry__._like_python(miss, pattern.encode(), escape.encode() if escape else None, ignore_case=True)
        assert oracle_keys.decrypt_char(run.words[name][0]) == want == 0, name


def test_exact_and_default_replay_decrypt_alike_and_differ_in_words(small, oracle_keys, oracle_sk):
    from oracle import dag_parity
    script, inputs, exact = small
    default = dag_parity.replay(script, inputs, oracle_sk, 3, exact=False)
    assert default.plan == exact.plan                        # one plan, executed two ways
    a, b = exact.words["contains_clear"], default.words["contains_clear"]
    assert oracle_keys.decrypt_char(a[0]) == oracle_keys.decrypt_char(b[0]) == 1
    for blk in range(4):
        assert oracle_keys.decrypt_block(a[0, blk]) == oracle_keys.decrypt_block(b[0, blk])
    bad = dag_parity.mismatches(exact.words, default.words)   # the flag comes out of the followers' level
    assert bad and all(name == "contains_clear" for name, *_ in bad), bad
    with pytest.raises(AssertionError, match="differ from the plan replay"):
        dag_parity.compare(exact, default, "default replay against exact replay")


def test_the_reporter_names_result_character_block_and_word(small):
    from oracle import dag_parity
    rng = np.random.default_rng(7)
    want = dict(small[2].words, text=rng.integers(0, 1 << 64, (3, 4, 2049), dtype=np.uint64))
    same = {k: v.copy() for k, v in want.items()}
    assert dag_parity.mismatches(want, same) == []
    dag_parity.compare(dag_parity.Outcome(want, {}, 0.0, {}), dag_parity.Outcome(same, {}, 0.0, {}), "equal")
    for name, ch, blk, word in (("text", 2, 1, 2048), ("text", 0, 3, 0), ("contains_clear", 0, 2, 1033)):
        got = {k: v.copy() for k, v in want.items()}
        got[name][ch, blk, word] ^= np.uint64(1)             # one bit of one word
        assert dag_parity.mismatches(want, got) == [(name, ch, blk, word, 1)]
        with pytest.raises(AssertionError) as err:
            dag_parity.compare(dag_parity.Outcome(want, {}, 0.0, {}), dag_parity.Outcome(got, {}, 0.0, {}), "script X, config Y")
        msg = str(err.value)
        assert "script X, config Y" in msg and "%s[%d] block %d: first at word %d" % (name, ch, blk, word) in msg
        assert "1 of 2049 words differ" in msg
    got = {k: v.copy() for k, v in want.items()}
    got["text"][1, 0, 5:9] += np.uint64(3)                   # several words: the first is named, all are counted
    assert dag_parity.mismatches(want, got) == [("text", 1, 0, 5, 4)]


def test_one_flipped_word_of_an_input_is_named_first(small, oracle_keys, oracle_sk):
    """the whole chain: the same script replayed on a text of which one mask word has its top bit flipped"""
    from oracle import dag_parity
    script, inputs, exact = small
    text = inputs["text"].copy()
    text[3, 2, 1033] ^= np.uint64(1 << 63)
    other = dag_parity.replay(script, dict(inputs, text=text), oracle_sk, 3)
    assert other.plan == exact.plan
    bad = dag_parity.mismatches(exact.words, other.words)
    assert bad[0] == ("text", 3, 2, 1033, 1) and [b[0] for b in bad].count("text") == 1, bad
    with pytest.raises(AssertionError, match=r"text\[3\] block 2: first at word 1033 .*, 1 of 2049 words differ"):
        dag_parity.compare(exact, other, "flipped input")


def test_the_guard_says_what_differs(small):
    from oracle import dag_parity
    exact = small[2]
    other = dag_parity.Outcome(exact.words, dict(exact.plan, launch_groups=[12, 6]), 0.0, {})
    dag_parity.guard(exact, exact)
    with pytest.raises(AssertionError, match=r"launch_groups: planner \[12, 5, 1\], device \[12, 6\]"):
        dag_parity.guard(exact, other, "script X")
