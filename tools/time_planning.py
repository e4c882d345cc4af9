#!/usr/bin/env python3
"""Host planning time of the engine on planner contexts (CPU only): the time from the first recorded op to the end of
flush() for replace 1025 / 5 / 5 (131 405 bootstraps), le on 4097 + 4097 characters, find_wide on 4097 / 4, split_at
with a u8 position on 512 characters, and like_clear, regex_clear and regex_find_clear on 256 characters, one JSON line
per process.

A/B of two builds of the library (profiles/r10_engine_refactor_ab.json, profiles/r17_strings_refactor_ab.json,
profiles/r25_strings_flag_algebra_ab.json): run this
in alternating fresh processes with FHS_LIB_PATH pointing at one build or the other.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from fhestring_amd.api import MyServerKey
    scenarios = {
        "replace_1025_5_5": lambda sk: (sk.replace, (sk.dummy_string(1025), sk.dummy_string(5), sk.dummy_string(5))),
        "le_4097": lambda sk: (sk.le, (sk.dummy_string(4097), sk.dummy_string(4097))),
        "find_wide_4097_4": lambda sk: (sk.find_wide, (sk.dummy_string(4097), sk.dummy_string(4))),
        "split_at_u8_512": lambda sk: (sk.split_at, (sk.dummy_string(512), sk.dummy_string(1)[0])),
        "like_clear_256": lambda sk: (sk.like_clear, (sk.dummy_string(256), "%quick%br_wn%fox")),
        "regex_clear_256": lambda sk: (sk.regex_clear, (sk.dummy_string(256), b"[A-Z]{2}-[0-9]+ (error|warn).*timeout")),
        "regex_find_clear_256": lambda sk: (sk.regex_find_clear, (sk.dummy_string(256), b"(error|warn): [a-z]+")),
    }
    out = {}
    for name, make in scenarios.items():
        sk = MyServerKey.planner()
        sk.set_mode(1)
        op, args = make(sk)
        sk.stats(reset=True)
        t0 = time.perf_counter()
        keep = op(*args)
        sk.flush()
        out[name + "_s"] = round(time.perf_counter() - t0, 4)
        out[name + "_pbs"] = sk.stats()["pbs_executed"]
        del keep
        sk.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
