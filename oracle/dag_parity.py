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

tests/test_dag_parity.py (no GPU), tests/test_dag_parity_device.py and smoke() of __graft_entry__.py use this.
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
    of its results (replay: the oracle's bootstraps included)"""

    def __init__(self, words, plan, seconds, facts, rotations=None, extractions=None):
        self.words, self.plan, self.seconds, self.facts = words, plan, seconds, facts
        self.rotations, self.extractions = rotations, extractions


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
        return Outcome(words, plan, dt, inputs["facts"], rot, ext)
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
    """-> (script, string_mode, inputs) of case A .. G or "small" (the shape smoke() uses: `zama!\\0` / `ma`)"""
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
