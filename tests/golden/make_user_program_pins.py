"""Generates tests/golden/user_program_pins.json: the refusals and the program texts (len, sha256) of every flag word and every launch
layout of the user problems, as the library answers them (tests/user_program_pins.py holds the sweeps).

    python tests/golden/make_user_program_pins.py

DATA only.  The fixture pins a refactor, so it is recorded from a build of the commit BEFORE the change it guards (DDP_AMD_LIB names that
library) and never from the code under test: tests/test_user_program_pins_cpu.py replays the sweeps against it.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ddp_amd import _lib  # noqa: E402
import user_program_pins as pins  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "user_program_pins.json")

def rows(d, row_of):
    """the items of a flat dict as JSON, one line per run of keys with the same row_of(key)"""
    out, last = [], None
    for k, v in d.items():
        item = "%s: %s" % (json.dumps(k), json.dumps(v))
        if out and row_of(k) == last:
            out[-1] += ", " + item
        else:
            out.append(item)
        last = row_of(k)
    return "{\n" + ",\n".join(out) + "\n}"


if __name__ == "__main__":
    rec = pins.record(_lib.lib())
    fix = pins.pack(rec)
    # a row of the layout sweep: one n under one flag word (every m); of the accepted texts: four flag words; a refusal: one message
    parts = ['"clock": ' + json.dumps(fix["clock"]), '"layout": ' + rows(fix["layout"], lambda k: (k.split()[0], k.split()[2]))]
    sweeps = []
    for key, r in fix["flags"].items():
        acc = r["accepted"]
        words = list(acc) if "same_as" not in acc else []
        sweeps.append('%s: {"accepted": %s,\n"refused": %s}' % (json.dumps(key), rows(acc, lambda k: words.index(k) // 4 if words else 0),
                                                                rows(r["refused"], lambda k: k)))
    parts.append('"flags": {\n' + ",\n".join(sweeps) + "\n}")
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
    for key, v in sorted(rec["flags"].items()):
        print(key, len(v["refused"]), "messages,", sum(len(w) for w in v["refused"].values()), "refused,", len(v["accepted"]), "accepted")
    print("layout", len(rec["layout"]), "clock", rec["clock"])
    print(_lib.LIB_PATH, "->", OUT, os.path.getsize(OUT), "bytes")
