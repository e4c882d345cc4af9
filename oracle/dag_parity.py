"""TEST INFRASTRUCTURE (like everything under oracle/): a fused DAG on the device, word for word against the plan replay.

One *script* -- a Python function that records string operations on a server key -- is applied twice: to the planner
context of a `PlanRun` with exact_extractions (oracle/plan_exec.py), and to a device context under the same keys.  Both
get the same ciphertexts and the same sequence of set_mode / set_rotation_sharing / submit / pump / flush calls.  If the
two contexts planned alike (`GUARD`: rotations, extractions, levels, noise figure, level widths, launch groups), every
result handle has exactly one correct content in each arithmetic, and `compare` asks for it: all 4 x 2049 words of every
character, pending linear combinations, plaintext blocks and kept intermediates included.  A decrypt check forgives any
error below 2^58 and cannot tell a block from another that holds the same message; this one cannot be satisfied by a
follower extracted from the wrong leader, a sum that read a block one launch early, or a block read where it used to be.

    script(sk, upload, inputs) -> {name: FheAsciiChar | FheString | list of FheAsciiChar}

`upload(array [n, 4, 2049])` places a string; `inputs` are the ciphertexts (made once) and the clear parameters.  A script
must not branch on the kind of context.  What it wants to tell the test goes into inputs["facts"], a dict.

tests/test_dag_parity.py (no GPU), tests/test_dag_parity_device.py, tests/test_sched_parity_device.py and smoke() of
__graft_entry__.py use this.
"""
import os
import time

import numpy as np

from .plan_exec import PlanRun

GUARD = ("pbs_executed", "pbs_extracted", "levels", "max_input_sum_c2")
ORACLE_MODE = {0: 0, 1: 3, 2: 4, 3: 5}               # device arithmetic -> the oracle mode with the same words


def threads():
    return min(16, os.cpu_count() or 1)


def encrypt(keys, data):
    """bytes -> [len, 4, 2049]"""
    return np.stack([keys.encrypt_char(b) for b in data])


def printable(rng, n, pad=1):
    """n printable ASCII characters from a seeded numpy generator, `pad` NULs behind them"""
    return bytes(int(v) for v in rng.integers(0x20, 0x7F, n)) + bytes(pad)


def plan_of(sk):
    st = sk.stats()
    return {"stats": {k: st[k] for k in GUARD}, "level_widths": sk.level_widths(), "launch_groups": sk.launch_groups()}


def _chars(v):
    return list(v.chars) if hasattr(v, "chars") else (list(v) if isinstance(v, (list, tuple)) else [v])


class Outcome:
    """words: {result name: [n_chars, 4, 2049] u64}; plan: what the guard compares; seconds: the script and the reading
    of its results (replay: the oracle's bootstraps included); user_tables (replay only): per launch group the
    user-table ids its rows name (PlanRun.user_tables)"""

    def __init__(self, words, plan, seconds, facts, rotations=None, extractions=None, user_tables=None):
        self.words, self.plan, self.seconds, self.facts = words, plan, seconds, facts
        self.rotations, self.extractions, self.user_tables = rotations, extractions, user_tables


def replay(script, inputs, oracle_sk, mode, string_mode=1, sharing=True, exact=True):
    """the script on a planner context, its plan trace executed by the CPU oracle in arithmetic `mode`"""
    run = PlanRun(oracle_sk, threads(), mode=mode, string_mode=string_mode, exact_extractions=exact)
    try:
        run.sk.ctx.set_rotation_sharing(sharing)
        run.sk.stats(reset=True)
        t0 = time.perf_counter()
        inputs = dict(inputs, facts={})
        res = script(run.sk, run.upload_string, inputs)
        plan = plan_of(run.sk)
        run.run()
        words = {name: np.stack([run.result_char(c) for c in _chars(v)]) for name, v in res.items()}
        dt = time.perf_counter() - t0
        rot = run.rotations if exact else plan["stats"]["pbs_executed"]
        ext = run.extractions if exact else plan["stats"]["pbs_extracted"]
        assert (rot, ext) == (plan["stats"]["pbs_executed"], plan["stats"]["pbs_extracted"]) and run.pbs == rot + ext
        del res
        return Outcome(words, plan, dt, inputs["facts"], rot, ext, run.user_tables)
    finally:
        run.close()


def on_device(script, inputs, sk, string_mode=1, sharing=True):
    """the script on a device context (MyServerKey with its keys loaded); every result downloaded"""
    sk.set_mode(string_mode)
    sk.ctx.set_rotation_sharing(sharing)
    sk.stats(reset=True)
    t0 = time.perf_counter()
    inputs = dict(inputs, facts={})
    res = script(sk, sk.upload_string, inputs)
    plan = plan_of(sk)
    words = {name: np.stack([c.download() for c in _chars(v)]) for name, v in res.items()}
    dt = time.perf_counter() - t0
    del res
    return Outcome(words, plan, dt, inputs["facts"])


def guard(want, got, what=""):
    """both contexts planned alike -- or the planner is not the stand-in for the device that the replay assumes"""
    diff = ["%s: planner %r, device %r" % (k, want.plan[k], got.plan[k]) for k in want.plan if want.plan[k] != got.plan[k]]
    assert not diff, "%s: planner and device context planned differently -- %s" % (what, "; ".join(diff))


def mismatches(want, got):
    """[(result, char, block, first differing word, number of differing words)] over every block of every result"""
    out = []
    assert sorted(want) == sorted(got), (sorted(want), sorted(got))
    for name in want:
        a, b = np.asarray(want[name]), np.asarray(got[name])
        assert a.shape == b.shape and a.dtype == b.dtype == np.uint64, (name, a.shape, b.shape)
        if np.array_equal(a, b):
            continue
        for ch, blk in zip(*np.nonzero((a != b).any(axis=2))):
            d = np.nonzero(a[ch, blk] != b[ch, blk])[0]
            out.append((name, int(ch), int(blk), int(d[0]), int(d.size)))
    return out


def compare(want, got, what=""):
    """every word of every result, np.array_equal; the message names script / configuration (`what`), result, character,
    block, first differing word and how many words differ"""
    bad = mismatches(want.words, got.words)
    if bad:
        lines = ["%s[%d] block %d: first at word %d (replay %#018x, device %#018x), %d of 2049 words differ" % (
            n, c, b, w, int(want.words[n][c, b, w]), int(got.words[n][c, b, w]), k) for n, c, b, w, k in bad[:12]]
        raise AssertionError("%s: %d block(s) differ from the plan replay\n  %s%s" % (
            what, len(bad), "\n  ".join(lines), "" if len(bad) <= 12 else "\n  ..."))


def check(script, inputs, want, sk, what, **kw):
    got = on_device(script, inputs, sk, **kw)
    guard(want, got, what)
    compare(want, got, what)
    return got


# ---- the cases: script, string mode, inputs (characters from a seeded generator, one NUL of padding each) ----------
def case(name, keys):
    """-> (script, string_mode, inputs) of case A .. L or "small" (the shape smoke() uses: `zama!\\0` / `ma`)"""
    rng = np.random.default_rng(0xDA6 + sum(name.encode()))
    put = lambda text, at, pat: text[:at] + pat + text[at + len(pat):]
    if name == "small":
        return contains_clear, 1, {"text": encrypt(keys, b"zama!\0"), "pattern": "ma", "clear": b"zama!\0"}
    if name == "A":                                          # 64 characters; the pattern's nibbles are all different
        return contains_clear, 1, {"text": encrypt(keys, put(printable(rng, 64), 41, b"Qz7#")), "pattern": "Qz7#"}
    if name in ("B", "F"):
        inp = {"text": encrypt(keys, put(printable(rng, 12), 5, b"k;W")), "pattern": encrypt(keys, b"k;W"), "count": 4}
        if name == "F":                                      # 500 characters of any words: 2000 of a chunk's 2048 blocks
            inp.update(trim=True, filler=rng.integers(0, 1 << 64, (500, 4, 2049), dtype=np.uint64))
        return find_then_positions, 1, inp
    if name == "C":
        text = put(printable(rng, 12), 3, b"A_c")
        return like_twice, 1, {"text": encrypt(keys, text), "like": "%a_c%", "like_escaped": "%a\\_c%", "escape": "\\",
                               "clear": text}
    if name in ("D", "E"):
        a = printable(rng, 16)
        b = bytearray(a.swapcase())                          # the other case throughout, one character different
        b[9] ^= 1
        inp = {"a": encrypt(keys, a), "b": encrypt(keys, bytes(b)), "clear": (a, bytes(b))}
        if name == "E":
            inp.update(text=encrypt(keys, put(printable(rng, 16), 7, b"Qz7#")), pattern="Qz7#")
        return (le_and_eq_ignore_case if name == "D" else two_jobs), 1, inp
    if name == "G":
        return eq_as_written, 0, {"a": encrypt(keys, b"fhe\0"), "b": encrypt(keys, b"fhf\0")}
    # H .. L, the scheduler's hazards: wherever it could confuse two strings they hold the same clear message under
    # fresh encryptions, so that only the words tell them apart
    if name == "H":                                          # 0 = 2 and 1 = 3 in the clear; the pattern in 0, 2 and 4
        hit, miss, hit4, miss5 = (printable(rng, 16) for _ in range(4))
        clear = [put(hit, 6, b"Qz7#"), miss, put(hit, 6, b"Qz7#"), miss, put(hit4, 11, b"Qz7#"), miss5]
        return skewed_requests, 1, {"texts": [encrypt(keys, t) for t in clear], "pattern": "Qz7#", "slots": 0, "clear": clear}
    if name == "I":
        a, d = printable(rng, 4, pad=0), printable(rng, 4, pad=0)
        return freed_under_a_scheduled_tick, 1, {"a": encrypt(keys, a), "d1": encrypt(keys, d), "d2": encrypt(keys, d),
                                                 "b": encrypt(keys, d), "c": encrypt(keys, d), "clear": (a, d)}
    if name == "J":
        a, b = b"hello world\0", b"HELLO WORLD\0"
        return job_consuming_an_unfinished_job, 1, {"a": encrypt(keys, a), "b": encrypt(keys, b), "pattern": "wor",
                                                    "clear": (a, b)}
    if name == "K":
        text, frm, to = b"ab~fcd~fgh\0\0", b"~f", b"[]"
        return auto_flush_peels, 1, {"text": encrypt(keys, text), "from": encrypt(keys, frm), "to": encrypt(keys, to),
                                     "threshold": 16, "clear": (text, frm, to)}
    if name == "L":                                          # 2 jobs: tests/test_dag_parity.py asserts that they suffice
        chars = [printable(rng, 1, pad=0) for _ in range(2)]
        tables = [bytes(int(v) for v in rng.integers(0, 256, 256)) for _ in chars]
        return tables_grow_under_scheduled_jobs, 1, {"chars": [encrypt(keys, c) for c in chars], "tables": tables,
                                                     "clear": chars}
    raise KeyError(name)


# ---- the scripts --------------------------------------------------------------------------------------------------
def contains_clear(sk, upload, inp):
    """A and the small shape: one fused contains_clear (rotation sharing, followers at K >= 2048 among them); the
    uploaded string is a result too -- blocks that nothing may have written"""
    s = upload(inp["text"])
    res = sk.contains_clear(s, inp["pattern"])
    sk.flush()
    return {"text": s, "contains_clear": res}


def find_then_positions(sk, upload, inp):
    """B, and F with inp["trim"]: find with an encrypted pattern, flush; its index -- unrefreshed sums -- as the encrypted
    position of char_at and substr, flush.  F: a filler string in front fills the first chunk of the block pool but for
    48 blocks, so that text and pattern straddle two chunks; it is dropped after the first flush and the pool compacted,
    which moves the live blocks of the emptier chunk: operands of the second flush."""
    filler = upload(inp["filler"]) if inp.get("trim") else None
    s, pat = upload(inp["text"]), upload(inp["pattern"])
    idx = sk.find(s, pat.chars)
    sk.flush()
    if inp.get("trim"):
        del filler
        inp["facts"].update(sk.pool_trim(compact=True))
    one, sub = sk.char_at(s, idx), sk.substr(s, idx, inp["count"])
    sk.flush()
    return {"find": idx, "char_at": one, "substr": sub, "text": s}


def like_twice(sk, upload, inp):
    """C: like_clear with ignore_case, without and with an escape byte -- two extractions of one rotation are added"""
    s = upload(inp["text"])
    a = sk.like_clear(s, inp["like"], ignore_case=True)
    b = sk.like_clear(s, inp["like_escaped"], escape=inp["escape"], ignore_case=True)
    sk.flush()
    return {"like": a, "like_escaped": b}


def le_and_eq_ignore_case(sk, upload, inp):
    """D: two operations that share their levels; negative and multi-term coefficients"""
    a, b = upload(inp["a"]), upload(inp["b"])
    le, eqi = sk.le(a, b), sk.eq_ignore_case(a, b)
    sk.flush()
    return {"le": le, "eq_ignore_case": eqi}


def two_jobs(sk, upload, inp):
    """E: D and a contains_clear as two submitted jobs whose rows ride in the same launch groups, one tick at a time"""
    sk.set_tick_balance(inp["slots"])
    try:
        a, b = upload(inp["a"]), upload(inp["b"])
        le, eqi = sk.le(a, b), sk.eq_ignore_case(a, b)
        sk.submit()
        s = upload(inp["text"])
        has = sk.contains_clear(s, inp["pattern"])
        sk.submit()
        while True:                                          # until a tick runs nothing
            n = len(sk.launch_groups())
            sk.pump(1)
            if len(sk.launch_groups()) == n:
                break
        sk.flush()
    finally:
        sk.set_tick_balance(0)
    return {"le": le, "eq_ignore_case": eqi, "contains_clear": has}


def eq_as_written(sk, upload, inp):
    """G (string mode 0): many narrow levels, nothing shared"""
    a, b = upload(inp["a"]), upload(inp["b"])
    res = sk.eq(a, b)
    sk.flush()
    return {"eq": res}


def skewed_requests(sk, upload, inp):
    """H, the benchmark's schedule in small: one request per tick -- contains_clear and to_upper of a string that the
    caller drops before the tick that reads it is enqueued -- drained by an asynchronous flush; the downloads
    synchronise.  to_upper's result keeps sharing the input's untouched blocks; contains_clear's inputs go back to the
    pool under scheduled ticks.  inp["slots"]: the tick balance (0: launch groups of up to three jobs' levels as they
    come; otherwise every first level is cut to whole rounds and its excess runs one tick later with its consumers)."""
    sk.set_tick_balance(inp["slots"])
    try:
        res = {}
        for k, text in enumerate(inp["texts"]):
            s = upload(text)
            res["contains_%d" % k], res["upper_%d" % k] = sk.contains_clear(s, inp["pattern"]), sk.to_upper(s)
            sk.submit()
            del s
            sk.pump(1)
        sk.flush(wait=False)
    finally:
        sk.set_tick_balance(0)
    return res


def freed_under_a_scheduled_tick(sk, upload, inp):
    """I: the inputs of a submitted job are released before any tick is enqueued, and two more strings are uploaded
    behind them: they must not get the blocks that the scheduled eq still has to read (BlockPool::free defers them).
    d1, d2, b and c hold one message, so both flags decrypt to 1 whichever blocks were read.  to_upper's result still
    refers to a's blocks, so dropping a returns nothing: facts["blocks_returned"] are d1's and d2's."""
    a, d1, d2 = upload(inp["a"]), upload(inp["d1"]), upload(inp["d2"])
    up, same_d = sk.to_upper(a), sk.eq(d1, d2)
    sk.submit()
    live = sk.stats()["blocks_live"]
    del a, d1, d2
    inp["facts"]["blocks_returned"] = live - sk.stats()["blocks_live"]
    b, c = upload(inp["b"]), upload(inp["c"])
    same = sk.eq(b, c)
    sk.submit()
    sk.flush()
    return {"up": up, "same_d": same_d, "same": same, "b": b, "c": c}


def job_consuming_an_unfinished_job(sk, upload, inp):
    """J: three jobs scheduled before anything is enqueued -- the second consumes every character of the first, the
    third is independent -- two ticks pumped, then an operation flushed in between, which drains what is scheduled"""
    a, b = upload(inp["a"]), upload(inp["b"])
    low = sk.to_lower(b)
    sk.submit()
    same = sk.eq(a, low)
    sk.submit()
    other = sk.contains_clear(a, inp["pattern"])
    sk.submit()
    sk.pump(2)
    mid = sk.len(a)
    sk.flush()
    return {"to_lower": low, "eq": same, "contains_clear": other, "len": mid}


AUTO_FLUSH_DEFAULT = 8192                                    # Engine::auto_flush_pending as a context is created


def auto_flush_peels(sk, upload, inp):
    """K: with fhs_set_auto_flush(inp["threshold"]) the ready level is peeled again and again while the DAGs are still
    being recorded: released pending nodes whose slots are reused, and an intermediate that is recorded, partly run and
    dropped.  Only a context that has never been driven with submit flushes on its own."""
    sk.set_auto_flush(inp["threshold"])
    try:
        text, frm, to = upload(inp["text"]), upload(inp["from"]), upload(inp["to"])
        rep = sk.replace(text, frm, to)
        tmp = sk.to_upper(text)
        del tmp
        pos = sk.rfind(text, frm.chars)
        sk.flush()
    finally:
        sk.set_auto_flush(AUTO_FLUSH_DEFAULT)
    return {"replace": rep, "rfind": pos}


def tables_grow_under_scheduled_jobs(sk, upload, inp):
    """L: map_clear of one character per job, each with a random 256-entry table of its own (about 64 user tables), one
    job per tick: the device array of table polynomials has to grow -- wait for the stream, move -- in front of a tick
    that has earlier ticks in the stream before it and scheduled ticks, which name their tables by id, behind it"""
    res = {}
    for k, (ch, table) in enumerate(zip(inp["chars"], inp["tables"])):
        s = upload(ch)
        res["map_%d" % k] = sk.map_clear(s, table)
        sk.submit()
        sk.pump(1)
    sk.flush()
    return res


# ---- reading a plan ---------------------------------------------------------------------------------------------------
def plan(script, inputs, string_mode=1, sharing=True):
    """what a planner context plans for the script (plan_of), nothing executed: the structural facts of a configuration
    whose words are not needed"""
    run = PlanRun(None, 1, string_mode=string_mode)
    try:
        run.sk.ctx.set_rotation_sharing(sharing)
        run.sk.stats(reset=True)
        res = script(run.sk, run.upload_string, dict(inputs, facts={}))
        out = plan_of(run.sk)
        del res
        return out
    finally:
        run.close()


def levels_by_group(plan):
    """the level widths of a plan, split by launch group: statistics note a tick's levels, then its group, so each group is
    the sum of the next few widths"""
    widths, out, i = plan["level_widths"], [], 0
    for g in plan["launch_groups"]:
        j = i
        while sum(widths[i:j]) < g and j < len(widths):
            j += 1
        assert sum(widths[i:j]) == g and j > i, (widths, plan["launch_groups"])
        out.append(widths[i:j])
        i = j
    assert i == len(widths), (widths, plan["launch_groups"])
    return out


def table_array_growth(user_tables, n_catalogue):
    """Engine::ensure_luts' rule over the launch groups of a replay (PlanRun.user_tables): the device array starts with
    room for the catalogue and grows, when a group names user tables it has no room for, to max(need, twice the room,
    catalogue + 64).  -> [(group, user tables resident before it, after it)] of every group at which it grows."""
    cap, seen, out = n_catalogue, set(), []
    for g, ids in enumerate(user_tables):
        need = n_catalogue + len(seen | ids)
        if need > cap:
            out.append((g, len(seen), len(seen | ids)))
            cap = max(need, 2 * cap, n_catalogue + 64)
        seen |= ids
    return out
