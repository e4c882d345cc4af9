"""The exact plan replay (PlanRun(exact_extractions=True): a shared extraction is read from its leader's accumulator, as
the device reads it) and the word-for-word comparison built on it (oracle/dag_parity.py), without a GPU.  The device
half is tests/test_dag_parity_device.py.

  * the exact replay in the f64-FFT mirror (oracle mode 3) decrypts like Python and like the regular expression;
  * negative control: exact and default replay (followers as bootstraps of their own) of one plan decrypt alike and
    differ in words -- which is what lets the device comparison tell "extracted from the leader" from "rotated on its
    own" (f64 arithmetic: the rounding of the FFT differs between the two accumulators; in exact arithmetic they agree
    except at decomposition ties, so nothing is asserted there);
  * the mismatch reporter names result, character, block and word;
  * scripts H .. L, the tick scheduler's hazards (device half: tests/test_sched_parity_device.py): every result of
    their replay decrypts to Python's answer, the plan has the property that makes the script worth running on the
    device, and a string swapped for another ciphertext of the same message is seen and named."""
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


# ---- scripts H .. L: the tick scheduler's hazards (the device half is tests/test_sched_parity_device.py) -------------
# Each is replayed once in oracle mode 3: every result decrypts to Python's answer, and the structural condition that
# makes the script worth running on the device is asserted on the plan itself.
def _text(keys, words):
    return bytes(keys.decrypt_char(w) for w in words)


@pytest.fixture(scope="module")
def freed(oracle_keys, oracle_sk):
    from oracle import dag_parity
    script, string_mode, inputs = dag_parity.case("I", oracle_keys)
    return script, inputs, dag_parity.replay(script, inputs, oracle_sk, 3, string_mode)


def test_requests_submitted_one_per_tick_share_launch_groups(oracle_keys, oracle_sk):
    """script H, the benchmark's schedule in small: 600 rotations + 468 extractions in 18 levels.  Tick balance off: the
    levels are 68 / 31 / 1 wide, the launch groups [68, 99, 100, 100, 100, 100, 32, 1] -- from the third tick on a group
    carries rows of three jobs.  Tick balance 48: groups [48, 96, 96, 96, 96, 96, 57, 15], no level as wide as in the
    other run -- every first level is split and its excess runs one tick later with its consumers."""
    from oracle import dag_parity
    script, string_mode, inputs = dag_parity.case("H", oracle_keys)
    clear = inputs["clear"]
    assert len(clear) == 6 and clear[0] == clear[2] and clear[1] == clear[3] and all(len(t) == 17 for t in clear)
    assert [b"Qz7#" in t for t in clear] == [True, False, True, False, True, False]
    run = dag_parity.replay(script, inputs, oracle_sk, 3, string_mode)
    for k, text in enumerate(clear):
        assert oracle_keys.decrypt_char(run.words["contains_%d" % k][0]) == int(inputs["pattern"].encode() in text), k
        assert _text(oracle_keys, run.words["upper_%d" % k]) == text.upper(), k
    assert (run.rotations, run.extractions, run.plan["stats"]["levels"]) == (600, 468, 18)
    by_group = dag_parity.levels_by_group(run.plan)
    assert sum(len(g) == 3 for g in by_group) >= 2, by_group     # three consecutive levels -- three jobs -- in one group
    balanced = dag_parity.plan(script, dict(inputs, slots=48), string_mode)
    assert balanced["stats"] == run.plan["stats"]
    groups = balanced["launch_groups"]
    assert len(groups) > 3 and all(g % 48 == 0 for g in groups[1:-2]), groups
    assert set(balanced["level_widths"]).isdisjoint(run.plan["level_widths"]), balanced["level_widths"]
    assert any(len(g) == 3 for g in dag_parity.levels_by_group(balanced))


def test_blocks_freed_under_a_scheduled_tick(freed, oracle_keys):
    """script I: 30 rotations in 4 levels, launch groups [24, 6]; the 32 blocks of d1 and d2 went back to the pool after
    their job was scheduled and before b and c were uploaded"""
    script, inputs, run = freed
    a, d = inputs["clear"]
    assert _text(oracle_keys, run.words["up"]) == a.upper()
    assert oracle_keys.decrypt_char(run.words["same_d"][0]) == int(d == d) == 1
    assert oracle_keys.decrypt_char(run.words["same"][0]) == 1
    assert _text(oracle_keys, run.words["b"]) == _text(oracle_keys, run.words["c"]) == d
    assert run.facts["blocks_returned"] == 32 == 2 * 4 * len(d)
    assert (run.rotations, run.plan["launch_groups"]) == (30, [24, 6])


def test_a_string_with_the_same_message_in_place_of_another_is_named(freed, oracle_keys, oracle_sk):
    """negative control of the hazard "a block is read where it used to be": script I with d1's own ciphertext uploaded
    as b, which is what a pool that handed d1's blocks out again early would amount to.  Every result decrypts as
    before; the words of `same` and of `b` do not, and the reporter names result, character, block and word."""
    from oracle import dag_parity
    script, inputs, run = freed
    other = dag_parity.replay(script, dict(inputs, b=inputs["d1"]), oracle_sk, 3)
    assert other.plan == run.plan
    for name in run.words:
        assert _text(oracle_keys, other.words[name]) == _text(oracle_keys, run.words[name]), name
    bad = dag_parity.mismatches(run.words, other.words)
    assert {b[0] for b in bad} == {"same", "b"}, bad
    name, ch, blk, word, n = bad[0]
    assert (name, ch) == ("same", 0) and n > 2000, bad[0]
    with pytest.raises(AssertionError, match=r"same\[0\] block %d: first at word %d .*, %d of 2049 words differ" % (blk, word, n)):
        dag_parity.compare(run, other, "d1's ciphertext as b")


def test_a_job_that_consumes_an_unfinished_job(oracle_keys, oracle_sk):
    """script J: 124 rotations + 28 extractions in 12 levels, launch groups [60, 22, 13, 12, 2, 1, 12, 2].  to_lower alone
    plans levels [24, 12], eq of a string with to_lower's result [12, 12, 12, 2, 1], contains_clear [24, 10, 1], len
    [12, 2].  to_lower changes one block of a character and shares the others with its input, so eq's first level -- it
    reads blocks that to_lower did not write -- rides in the first tick with both other jobs; its second level, the
    first that reads what to_lower's last level (tick 2) writes, lands on tick 3: tick 2 carries no row of eq.  Two
    ticks are pumped, len is planned by the flush behind the ticks it drains."""
    from oracle import dag_parity
    script, string_mode, inputs = dag_parity.case("J", oracle_keys)
    a, b = inputs["clear"]
    run = dag_parity.replay(script, inputs, oracle_sk, 3, string_mode)
    assert _text(oracle_keys, run.words["to_lower"]) == b.lower() == a
    assert oracle_keys.decrypt_char(run.words["eq"][0]) == int(a == b.lower()) == 1
    assert oracle_keys.decrypt_char(run.words["contains_clear"][0]) == int(inputs["pattern"].encode() in a) == 1
    assert oracle_keys.decrypt_char(run.words["len"][0]) == len(a.rstrip(b"\0")) == 11
    assert (run.rotations, run.extractions, run.plan["stats"]["levels"]) == (124, 28, 12)

    def alone(op):                                           # the levels of one operation planned by itself
        def one(sk, upload, inp):
            x, y = upload(inp["a"]), upload(inp["b"])
            res = op(sk, x, y)
            sk.flush()
            return {"res": res}
        return dag_parity.plan(one, inputs, string_mode)["level_widths"]

    def lower_then_eq(sk, x, y):
        low = sk.to_lower(y)
        sk.flush()
        return sk.eq(x, low)

    lower, both = alone(lambda sk, x, y: sk.to_lower(y)), alone(lower_then_eq)
    assert both[:len(lower)] == lower
    eq = both[len(lower):]
    has, length = alone(lambda sk, x, y: sk.contains_clear(x, inputs["pattern"])), alone(lambda sk, x, y: sk.len(x))
    assert len(lower) == 2 and len(eq) > 2 and len(has) == 3
    by_group = dag_parity.levels_by_group(run.plan)
    assert by_group[0] == [lower[0], eq[0], has[0]]          # tick 1: the first level of every job
    assert by_group[1] == [lower[1], has[1]]                 # tick 2: to_lower's last level, and no row of eq
    assert by_group[2] == [eq[1], has[2]]                    # tick 3: eq goes on behind to_lower's last tick
    assert by_group[3:] == [[w] for w in eq[2:] + length]    # the rest of eq drained by the flush, then len


def test_automatic_partial_flush_peels_the_ready_level(oracle_keys, oracle_sk):
    """script K, threshold 16: 657 rotations in 35 launch groups, the widest 65 rows; the same script with automatic
    flushes off plans 17 levels (575 rotations: the dropped to_upper never runs)"""
    from oracle import dag_parity
    script, string_mode, inputs = dag_parity.case("K", oracle_keys)
    text, frm, to = inputs["clear"]
    run = dag_parity.replay(script, inputs, oracle_sk, 3, string_mode)
    assert _text(oracle_keys, run.words["replace"]).rstrip(b"\0") == text.rstrip(b"\0").replace(frm, to) == b"ab[]cd[]gh"
    assert oracle_keys.decrypt_char(run.words["rfind"][0]) == text.rfind(frm) == 6
    assert inputs["threshold"] == 16 and (run.rotations, max(run.plan["level_widths"])) == (657, 65)
    off = dag_parity.plan(script, dict(inputs, threshold=0), string_mode)
    assert len(run.plan["launch_groups"]) > off["stats"]["levels"] > 0, (run.plan["launch_groups"], off)


def test_the_table_array_grows_under_scheduled_jobs(oracle_keys, oracle_sk):
    """script L with two jobs: 296 rotations, launch groups [80, 144, 68, 4].  The first level of a map_clear with a
    random table names 80 user tables, 64 of them its own: the array of table polynomials, which starts with room for
    the catalogue's 71 alone, grows in front of the first tick to hold those 80 -- and again in front of the second (80
    tables resident, 144 needed), with the first tick in the stream and two more ticks scheduled behind it.  With one
    job the only tick that names a new table is the first one."""
    import fhestring_amd
    from oracle import dag_parity
    script, string_mode, inputs = dag_parity.case("L", oracle_keys)
    assert len(inputs["chars"]) == 2
    run = dag_parity.replay(script, inputs, oracle_sk, 3, string_mode)
    for k, (ch, table) in enumerate(zip(inputs["clear"], inputs["tables"])):
        assert _text(oracle_keys, run.words["map_%d" % k]) == ch.translate(table), k
    n_groups = len(run.plan["launch_groups"])
    assert len(run.user_tables) == n_groups
    grows = dag_parity.table_array_growth(run.user_tables, fhestring_amd.lib().fhs_lut_catalogue_count())
    middle = [(g, before, after) for g, before, after in grows if 0 < g < n_groups - 1]
    assert middle and all(before > 0 for _, before, _ in middle), grows   # tables in use move with the array
