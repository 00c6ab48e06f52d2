"""records_to_edges_sorted (lds_count.hip), the counting primitive of every build, on record arrays of the tests' own making through
katome_dev_count_records, each LDS strategy against a dictionary (tests/count_model.py): u32 weights of every size and sums that
wrap, the threshold at its boundary with the doubled weight of a self-complementary k-mer, the extremes of the key range, the salt of
the whole-key slots as a key word, records without weights, a group beyond the fingerprint slots' 20 bits, nothing and one record,
and the owner split.  Every case compares the WHOLE sorted output list with the model's, so that a key that left twice with partial
counts fails, and n_out and n_distinct with it.  The cases: tests/count_records_cases.py.

The switches are read once per process, so the cases run in one child process per set of switches, every child under its own time
limit and with KATOME_LC_TRACE=1; from its stderr, case by case, the parent holds the [lds count] lines against the ones the set
must give -- the kernel that was to count the case did, and said the code it was to say; a silent way round does not pass.

What these sizes cannot reach (nothing here forces it either): more than one sub-round of the 12-byte slots and their table of 13
slots per thread (groups of more than 5800 records: 380 M records), more than one visit of the 8-byte slots, the optimistic first
attempt (code 3) and the larger whole-key table after the small one filled."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "count_records_cases.py")
SWITCHES = ("KATOME_LC_PACKED", "KATOME_LC_FULL", "KATOME_LC_FULL_PER", "KATOME_LC_PROBE_LIMIT", "KATOME_LC_OPTIMISM")
SETS = {
    "default": {},
    "packed_always": {"KATOME_LC_PACKED": "2"},
    "packed_never": {"KATOME_LC_PACKED": "0"},
    "whole_keys_7": {"KATOME_LC_FULL": "1", "KATOME_LC_FULL_PER": "7"},
    "whole_keys_4": {"KATOME_LC_FULL": "1", "KATOME_LC_FULL_PER": "4"},
    "whole_keys_never": {"KATOME_LC_FULL": "0"},
}
SAMPLED_FROM = 1 << 16          # records from which the default route counts 256 groups of a two- or three-word level to choose its kernel

_RUNS = {}


class Run:
    def __init__(self, switches, out):
        self.switches = switches
        self.rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
        self.trace = {}
        for part in out.stderr.split("CASE ")[1:]:
            name, _, rest = part.partition("\n")
            self.trace[name] = [line for line in rest.splitlines() if line.startswith("[lds count]")]
        self.by_name = {r["name"]: r for r in self.rows}


@pytest.fixture(scope="module", params=list(SETS))
def run(request):
    """one child per set of switches, started when the set's first test asks for it; a child that does not end with status 0 (a
    status no case expects, a fault, the time limit) fails every test of its set and is not started again"""
    name = request.param
    if name not in _RUNS:
        env = dict(os.environ, KATOME_LC_TRACE="1")
        for s in SWITCHES:
            env.pop(s, None)
        env.update(SETS[name])
        try:
            out = subprocess.run([sys.executable, CHILD, ROOT], env=env, capture_output=True, text=True, timeout=240)
            _RUNS[name] = Run(SETS[name], out) if out.returncode == 0 else (out.returncode, out.stdout[-1500:], out.stderr[-3000:])
        except subprocess.TimeoutExpired as e:
            _RUNS[name] = ("time limit", str(e.stdout)[-1500:], str(e.stderr)[-3000:])
    assert isinstance(_RUNS[name], Run), (name,) + _RUNS[name]
    return _RUNS[name]


def _s12(code):
    return "[lds count] 12-byte slots, 1 sub-round(s): code %d" % code


def _s8(code):
    return "[lds count] 8-byte slots, 1 visit(s) per record: code %d" % code


_S8_GAVE_UP = "[lds count] 8-byte slots: a count beyond 16 bits; counting with the 12-byte slots"


def _whole(nw, per, code):
    return "[lds count] whole %skeys in the slots (%d per thread): code %d" % ("three-word " if nw == 3 else "", per, code)


def expected_trace(switches, c):
    """the [lds count] lines a case must leave under a set of switches, in order; a list of alternatives where the set leaves one open"""
    if c["n"] == 0 or c["status"] == "E_ARG" or c["expect"] == "E_UNSUPPORTED":
        return [[]]                                         # (refused, or nothing to count: no kernel ran)
    nw, split = c["nw"], c["n_parts"] > 0
    last = [_s12(4 if c["huge"] else 0)]
    if nw >= 2:
        full = switches.get("KATOME_LC_FULL")
        if full == "1":
            per = {(2, "7"): 7, (2, "4"): 4, (3, "7"): 5, (3, "4"): 3}[(nw, switches["KATOME_LC_FULL_PER"])]
            return [[_whole(nw, per, 7)] + last] if c["salt"] else [[_whole(nw, per, 0)]]
        if full is None and c["n"] >= SAMPLED_FROM:
            # groups of a few distinct keys: the sample takes the small table.  A salt word may already meet the sample, which then says no
            per = 4 if nw == 2 else 3
            return [[_whole(nw, per, 7)] + last, last] if c["salt"] else [[_whole(nw, per, 0)]]
        return [last]
    if switches.get("KATOME_LC_PACKED") == "2" and not split and c["weights"] and not (c["rc"] and c["k"] % 2 == 0):
        return [[_s8(5), _S8_GAVE_UP] + last] if c["over16"] else [[_s8(0)]]
    return [last]


def test_every_case_ran(run):
    names = [r["name"] for r in run.rows]
    assert len(names) == len(set(names)) and len(names) >= 120 and names[-1] == "arguments", names
    for prefix, at_least in (("uniform_", 12), ("all64_", 2), ("ladder", 9), ("sums_", 15), ("threshold", 40), ("extremes_", 8), ("salt", 11), ("unit_", 7),
                             ("huge_group", 1), ("n0_", 3), ("n1_", 4), ("owners_", 9)):
        assert sum(1 for n in names if n.startswith(prefix)) >= at_least, prefix
    assert {r["k"] for r in run.rows if "k" in r} >= {3, 16, 31, 32, 40, 63, 64, 95}
    for r in run.rows:
        assert r["n"] <= 2_500_000


def test_every_list_is_the_models(run):
    """the comparisons are the child's: the whole sorted list, n_out, n_distinct; per owner with a split"""
    bad = [(r["name"], r.get("status"), r.get("detail"), r.get("message")) for r in run.rows if not r["ok"]]
    assert not bad, bad[:8]
    for r in run.rows:
        assert r["status"] == r["expect"] or r["huge"], r["name"]


def test_the_strategy_of_the_set_counted_every_case(run):
    for c in run.rows[:-1]:
        assert run.trace[c["name"]] in expected_trace(run.switches, c), (c["name"], run.trace[c["name"]], expected_trace(run.switches, c))


def test_the_give_up_codes_are_met(run):
    """the sets that force a slot shape meet its give-up path at least where the issue names it: a count beyond 16 bits (code 5) on
    the weight ladder and the sums, the salt word (code 7) as second word of two- and three-word keys -- and come out right (above)"""
    said = [line for lines in run.trace.values() for line in lines]
    if run.switches.get("KATOME_LC_PACKED") == "2":
        for name in ("ladder_k16_t0", "ladder_rc_k31_t1", "sums_carry_k16", "sums_carry_k31", "sums_wrap_k16", "sums_wrap_k31_t1"):
            assert run.trace[name][:2] == [_s8(5), _S8_GAVE_UP], name
        for name in ("sums_fit_k16", "sums_fit_k31", "uniform_k31", "uniform_rc_k31_t3", "all64_k3", "all64_rc_k3_t2", "extremes_k3", "extremes_k31"):
            assert run.trace[name] == [_s8(0)], name
        assert run.trace["uniform_rc_k16_t3"] == [_s12(0)]               # (even k on both strands stays with the 12-byte slots)
    else:
        assert not any("8-byte slots" in line for line in said)
    if run.switches.get("KATOME_LC_FULL") == "1":
        per2, per3 = (7, 5) if run.switches["KATOME_LC_FULL_PER"] == "7" else (4, 3)
        for name in ("salt_k32", "salt_k40", "salt_rc_k40", "salt_k63", "salt_rc_k63"):
            assert run.trace[name] == [_whole(2, per2, 7), _s12(0)], name
        for name in ("salt_second_k64", "salt_second_k95", "salt_third_own_k64", "salt_third_own_k95"):
            assert run.trace[name] == [_whole(3, per3, 7), _s12(0)], name
        for name in ("salt_third_k64", "salt_third_k95"):                # (the third word has a salt of its own)
            assert run.trace[name] == [_whole(3, per3, 0)], name
        assert sum(1 for line in said if line == _whole(2, per2, 0)) >= 30 and sum(1 for line in said if line == _whole(3, per3, 0)) >= 10
    if run.switches.get("KATOME_LC_FULL") == "0":
        assert not any("in the slots (" in line for line in said)


def test_a_group_beyond_20_bits(run):
    """the fingerprint slots name a group's representative in 20 bits: a group of 2^20 + 1 records is code 4 and KATOME_E_UNSUPPORTED,
    and the hash table, where a build counts the level then, gives the model's list; the whole-key slots count it as it is"""
    c = run.by_name["huge_group_k40"]
    assert c["n"] > (1 << 20) + 45000 and c["ok"]          # (2^20 + 1 of one key among some 50 000 others)
    if run.switches.get("KATOME_LC_FULL") == "0":
        assert c["status"] == "E_UNSUPPORTED" and "a group of more than 2^20 records" in c["message"] and c["route"] == "table"
        assert run.trace[c["name"]] == [_s12(4)]
    else:
        assert c["status"] == "OK" and c["n_out"] == c["n_distinct"] and "whole keys in the slots" in run.trace[c["name"]][0]


def test_the_owner_split_and_what_is_refused(run):
    for parts in (1, 2, 3, 8, 16):
        c = run.by_name["owners_%d" % parts]
        assert c["status"] == "OK" and c["ok"] and c["owners_used"] == parts and c["n_out"] == c["n_distinct"]
    for name in ("owners_17_refused", "owners_rc_refused", "owners_threshold_refused", "owners_two_words_refused", "unit_one_word_refused"):
        assert run.by_name[name]["status"] == "E_ARG", name
    for name in ("three_words_rc_refused", "three_words_threshold_refused"):
        assert run.by_name[name]["status"] == "E_UNSUPPORTED", name
    args = run.by_name["arguments"]
    assert args["ok"], args["got"]
