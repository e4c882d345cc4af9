#!/usr/bin/env python3
"""Host planning time of the engine on planner contexts (CPU only): the time from the first recorded op to the end of
flush() for replace 1025 / 5 / 5 (131 405 bootstraps) and le on 4097 + 4097 characters, one JSON line per process.

A/B of two builds of the library (profiles/r10_engine_refactor_ab.json): run this in alternating fresh processes with
FHS_LIB_PATH pointing at one build or the other.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from fhestring_amd.api import MyServerKey
    out = {}
    for name in ("replace_1025_5_5", "le_4097"):
        sk = MyServerKey.planner()
        sk.set_mode(1)
        if name.startswith("replace"):
            args = (sk.dummy_string(1025), sk.dummy_string(5), sk.dummy_string(5))
            op = sk.replace
        else:
            args = (sk.dummy_string(4097), sk.dummy_string(4097))
            op = sk.le
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
