"""The input space of validate + program_text (csrc/user_program.hip), swept through the two debug hooks ddp_user_program_text and
ddp_user_program_text_c: what tests/golden/make_user_program_pins.py records and tests/test_user_program_pins_cpu.py replays.  Nothing
is compiled: the stub source only holds the identifiers validate looks for.

    flag sweep    every flag word over the assigned bits and the unassigned bit 64, at a lane shape and a wave-capable shape, through both
                  hooks (the first with no constraint count, the second with nc = 2 under DDP_USER_CONSTRAINTS and 0 without it).  A
                  refused word is kept under the exact text of ddp_last_error (the word itself, where the message prints it, written
                  as {flags:x}), an accepted one as (len, sha256) of its program.
    layout sweep  every DDP_*LANES, DDP_*CHUNK, DDP_CSB, DDP_ADJ, DDP_ADH and DDP_WG is a #define of the text, so one digest per shape
                  pins layout_of; a shape refused for its LDS is kept under its message.
    clock         one DDP_USER_CLOCK program (the rewriter with_clock) with a non-zero diff_wrap.
"""
import hashlib

TERMINAL, CONST_HESSIAN, AUTODIFF, PLANT, SECOND, WAVE, SECOND_WAVE = 1, 2, 4, 8, 16, 32, 128
CLOCK, CONSTRAINTS, SAMPLE, FITTED, COST_FIT = 512, 1024, 2048, 4096, 8192
BITS = (TERMINAL, CONST_HESSIAN, AUTODIFF, PLANT, SECOND, WAVE, 64, SECOND_WAVE, CLOCK, CONSTRAINTS, SAMPLE, FITTED, COST_FIT)
NPARAM = 3
FLAG_SHAPES = ((4, 2), (16, 8))
LANE_FLAGS = TERMINAL | SAMPLE | FITTED | COST_FIT
WAVE_FLAGS = AUTODIFF | WAVE
CLOCK_CASE = (4, 2, TERMINAL | AUTODIFF | PLANT | CLOCK, 0x5)

STUB = b"""// a source that defines nothing: the names are all validate reads
// dynamics stage_cost derivatives terminal_cost cost_hessians plant constraints
struct ddp_stub { int dynamics, stage_cost, derivatives, terminal_cost, cost_hessians, plant, constraints; };
"""


def flag_words():
    for k in range(1 << len(BITS)):
        yield sum(b for i, b in enumerate(BITS) if k >> i & 1)


def _digest(text):
    return [len(text), hashlib.sha256(text).hexdigest()]


def _one(L, n, m, flags, wrap=0, nc=None):
    """(None, digest) of the program, or (message, None) where the arguments are refused"""
    if nc is None:
        text = L.ddp_user_program_text(STUB, n, m, NPARAM, flags, wrap)
    else:
        text = L.ddp_user_program_text_c(STUB, n, m, NPARAM, nc, flags, wrap)
    if text is None:                                             # (a message that prints the flag word: one key for all of them)
        return L.ddp_last_error().decode().replace("flags 0x%x" % flags, "flags 0x{flags:x}"), None
    return None, _digest(text)


def _ranges(words):
    """sorted ints as "a-b c d-e" """
    out, words = [], sorted(words)
    i = 0
    while i < len(words):
        j = i
        while j + 1 < len(words) and words[j + 1] == words[j] + 1:
            j += 1
        out.append(str(words[i]) if i == j else "%d-%d" % (words[i], words[j]))
        i = j + 1
    return " ".join(out)


def _words(ranges):
    out = []
    for part in ranges.split():
        a, _, b = part.partition("-")
        out.extend(range(int(a), int(b or a) + 1))
    return out


def pack(rec):
    """record() as the fixture file holds it, without loss: word lists as ranges, a digest as "len:sha256", and a sweep that repeats an
    earlier one (the refusals of the second shape; the texts of the hook without nc, which are those of the hook with it) as a reference"""
    dig = lambda v: "%d:%s" % tuple(v) if isinstance(v, list) else v
    out = {"flags": {}, "layout": {k: dig(v) for k, v in rec["layout"].items()}, "clock": {k: dig(v) for k, v in rec["clock"].items()}}
    for key in sorted(rec["flags"], reverse=True):               # (program_text_c first: the other hook refers to it)
        r = rec["flags"][key]
        refused = {msg: _ranges(ws) for msg, ws in r["refused"].items()}
        accepted = {w: dig(v) for w, v in r["accepted"].items()}
        for other, o in out["flags"].items():
            if isinstance(refused, dict) and o["refused"] == refused:
                refused = {"same_as": other}
            full = o["accepted"]
            if isinstance(accepted, dict) and "same_as" not in full and all(full.get(w) == v for w, v in accepted.items()):
                accepted = {"same_as": other, "words": _ranges(int(w) for w in accepted)}
        out["flags"][key] = {"refused": refused, "accepted": accepted}
    return out


def unpack(fix):
    """the inverse of pack()"""
    und = lambda v: [int(v.split(":")[0]), v.split(":")[1]] if v.split(":")[0].isdigit() else v
    out = {"flags": {}, "layout": {k: und(v) for k, v in fix["layout"].items()}, "clock": {k: und(v) for k, v in fix["clock"].items()}}
    for key in sorted(fix["flags"], reverse=True):
        r = fix["flags"][key]
        refused, accepted = r["refused"], r["accepted"]
        if "same_as" in refused:
            refused = out["flags"][refused["same_as"]]["refused"]
        else:
            refused = {msg: _words(ws) for msg, ws in refused.items()}
        if "same_as" in accepted:
            accepted = {str(w): out["flags"][accepted["same_as"]]["accepted"][str(w)] for w in _words(accepted["words"])}
        else:
            accepted = {w: und(v) for w, v in accepted.items()}
        out["flags"][key] = {"refused": refused, "accepted": accepted}
    return out


def record(L):
    """the whole record (JSON: every key a string)"""
    out = {"flags": {}, "layout": {}}
    for n, m in FLAG_SHAPES:
        for hook in ("program_text", "program_text_c"):
            refused, accepted = {}, {}
            for w in flag_words():
                nc = None if hook == "program_text" else (2 if w & CONSTRAINTS else 0)
                err, dig = _one(L, n, m, w, 0, nc)
                if err is None:
                    accepted[str(w)] = dig
                else:
                    refused.setdefault(err, []).append(w)
            out["flags"]["%s n=%d m=%d" % (hook, n, m)] = {"refused": refused, "accepted": accepted}
    shapes = [(n, m, f) for f in (LANE_FLAGS, LANE_FLAGS | CONST_HESSIAN) for n in range(1, 33) for m in range(1, 9)]
    shapes += [(n, m, f) for f in (WAVE_FLAGS, WAVE_FLAGS | SECOND_WAVE) for n in (1, 8, 33, 64) for m in (1, 8, 9, 16, 17, 32)]
    for n, m, f in shapes:
        err, dig = _one(L, n, m, f)
        out["layout"]["n=%d m=%d flags=%d" % (n, m, f)] = dig if err is None else err
    n, m, f, wrap = CLOCK_CASE
    err, dig = _one(L, n, m, f, wrap)
    out["clock"] = {"n=%d m=%d flags=%d wrap=%d" % (n, m, f, wrap): dig if err is None else err}
    return out
