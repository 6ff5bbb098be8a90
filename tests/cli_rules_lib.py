"""The command line's option rules as a recorded table (tests/test_cli_rules_cpu.py replays it).

Which refusal a command line gets - the wording, and WHICH one when it breaks several rules - is behaviour: scripts and
the option tests of every mode read it.  cases() spells a few thousand command lines out of one valid token per option
and the invalid arguments of every valued one; run_case() runs one of them with an empty stdin in an empty directory
against a database that does not exist, so a command line that passes every rule ends at "ERROR opening db file" or
"ERROR reading dbfilename from stdin" - before any device call: every case exits with status 1 and none prints
"found N HIP devices" (record() and the test both check that).

Two recordings lie in tests/golden/cli_rules/: normal.json from the package's command line, and stub.json from the
command line linked against tests/native/gpu_stubs.c, where the weak entry points are absent - the only build that
reaches the "this library has no ..." lines and shows their place in the order.  A recording is
{"texts": [[status, stderr], ...], "cases": {argument string: index into texts}}; in stderr the usage block is the
token <USAGE> (the block itself: usage.txt, once) and argv[0] is `satabsearch`.

    python tests/cli_rules_lib.py record      # rewrites the three files from the binaries of the working tree
"""
import itertools
import json
import os
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_rules")
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
STUB_SOURCES = [os.path.join(HOST, f) for f in ("sat_main.c", "sat_host_search.c", "sat_parse.c", "sat_gumbel.c", "sat_shard.c")] + \
               [os.path.join(ROOT, "tests", "native", "gpu_stubs.c")]

# one valid spelling of every option
VALID = [("-c",), ("-q", "nosuch.db"), ("-Q", "nosuch.db"), ("-a", "nosuch.db"), ("-r", "16"), ("-g", "1"), ("-G", "0,0"),
         ("-s", "7"), ("-b",), ("-k", "3"), ("-p", "0.5"), ("-m", "2"), ("-M", "2"), ("-R", "64"), ("-C", "5"), ("-F", "0.05"),
         ("-P", "2"), ("-A",), ("-L", "0.001"), ("-H", "0.001,0.01"), ("-E", "nosuch.cls"), ("-N", "5"), ("-D", "0.001"),
         ("-W", "0.001"), ("-f", "0.5"), ("-X", "0.01"), ("-x", "c")]

# the invalid arguments of every valued option: empty, text, trailing text, out of range on each side; nan / inf
_REAL = ["", "abc", "0.5x", "-0.1", "1.5", "nan", "inf", "-inf"]
_INT = ["", "abc", "2x", "0", "-1", "17", "2147483648", "99999999999999999999"]
INVALID = {"-p": _REAL, "-L": _REAL, "-D": _REAL, "-W": _REAL, "-X": _REAL, "-f": _REAL + ["0"], "-F": _REAL + ["0.6"],
           "-m": _INT, "-M": _INT, "-P": _INT, "-N": _INT, "-R": _INT, "-C": _INT,
           "-r": _INT[:3], "-g": _INT[:3], "-G": _INT[:3], "-s": _INT[:3], "-k": _INT[:5],
           "-q": [""], "-Q": [""], "-a": [""], "-E": [""],
           "-H": ["", "abc", "0.001x", "-0.1,0.5", "0.5,1.5", "nan", "0.1,inf", "0.01,0.001", "0.01,0.01", "0.001,,0.01", "0.001,",
                  ",0.001", "0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9"],
           "-x": ["", "abc", "cx", "S"]}


def _with(base, size):
    """every set of `size` valid tokens that contains the tokens of `base`, in VALID's order"""
    rest = [t for t in VALID if t not in base]
    for extra in itertools.combinations(rest, size - len(base)):
        yield [t for t in VALID if t in base or t in extra]


def cases():
    """The command lines, each a list of arguments; no two alike"""
    by_letter = {t[0]: t for t in VALID}
    sets = [[t] for t in VALID]
    sets += [[(letter, arg)] for letter, args in INVALID.items() for arg in args]
    sets += _with([], 2)
    sets += _with([by_letter["-a"]], 3)
    sets += _with([by_letter["-a"], by_letter["-p"]], 4)
    sets += _with([by_letter["-a"], by_letter["-P"], by_letter["-A"]], 4)
    sets += _with([by_letter["-k"], by_letter["-R"]], 4)
    seen, out = set(), []
    for s in sets:
        args = [a for t in s for a in t]
        if tuple(args) not in seen:
            seen.add(tuple(args))
            out.append(args)
    return out


def build_stub(out_dir):
    """The command line linked against the stubs of the device library: plain gcc, no sanitizer"""
    binary = os.path.join(str(out_dir), "satabsearch_stub")
    subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", binary] +
                   STUB_SOURCES + ["-lm", "-lpthread"], check=True)
    return binary


def _split_usage(err, binary):
    """stderr with argv[0] normalised and the usage block - from its "Usage:" line to its last line, which ends the
    text - cut out: (the rest with <USAGE> in its place, the block or None)"""
    err = err.replace(binary, "satabsearch")
    at = err.find("Usage: satabsearch ")
    if at < 0:
        return err, None
    return err[:at] + "<USAGE>\n", err[at:]


def run_case(binary, args, cwd):
    p = subprocess.run([binary, *args], stdin=subprocess.DEVNULL, cwd=cwd, capture_output=True, timeout=60)
    assert p.stdout == b"", (args, p.stdout[:200])
    return (p.returncode,) + _split_usage(p.stderr.decode(), binary)


def run_all(binary):
    """{argument string: (status, stderr)} of every case, and the usage block - the same wherever it is printed"""
    todo = cases()
    with tempfile.TemporaryDirectory() as cwd, ThreadPoolExecutor(max_workers=8) as pool:
        results = list(pool.map(lambda args: run_case(binary, args, cwd), todo))
        assert os.listdir(cwd) == [], "a case wrote a file"
    usages = {u for _, _, u in results if u is not None}
    assert len(usages) == 1, "the usage text differs between cases"
    out = {}
    for args, (status, err, _) in zip(todo, results):
        # no case gets as far as a device: the rules, then the missing database
        assert status == 1 and "HIP devices" not in err, (args, status, err)
        out[shlex.join(args)] = (status, err)
    return out, usages.pop()


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        rec = json.load(f)
    return {k: tuple(rec["texts"][i]) for k, i in rec["cases"].items()}


def load_usage():
    with open(os.path.join(GOLDEN, "usage.txt")) as f:
        return f.read()


def record():
    os.makedirs(GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        runs = {"normal": run_all(CLI), "stub": run_all(build_stub(d))}
    assert runs["normal"][1] == runs["stub"][1]
    with open(os.path.join(GOLDEN, "usage.txt"), "w") as f:
        f.write(runs["normal"][1])
    for name, (outcomes, _) in runs.items():
        texts = sorted(set(outcomes.values()))
        index = {t: i for i, t in enumerate(texts)}
        with open(os.path.join(GOLDEN, name + ".json"), "w") as f:
            json.dump({"texts": texts, "cases": {k: index[v] for k, v in outcomes.items()}}, f, separators=(",", ":"))
            f.write("\n")
        print(f"{name}: {len(outcomes)} cases, {len(texts)} distinct outcomes")


if __name__ == "__main__":
    if sys.argv[1:] != ["record"]:
        sys.exit(__doc__)
    record()
