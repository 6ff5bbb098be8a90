"""Motif queries without a GPU: the list parser (in the host library, and under the sanitizers in a stand-alone
program), the command line's -c -q with SID@list lines against -c on a stand-alone query file of the same
sub-structures, the blocks that must not change, the refusals, the usage text and the declarations."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cuda_satabsearch_amd as sat
from cuda_satabsearch_amd import _native
import edge_cases as ec
import motif_lib as ml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_satabsearch_amd", "bin", "satabsearch")
HOST = os.path.join(ROOT, "cuda_satabsearch_amd", "csrc", "host")
BLOCK = b"# cudaSaTabsearch"


def run(golden_dir, args, stdin=b""):
    return subprocess.run([CLI] + args, input=stdin, cwd=golden_dir, capture_output=True, timeout=300)


def parse(text, order):
    """(the 1-based list, None) or (None, the message) of sat_parse_sse_list"""
    host = _native.host_lib()
    host.sat_parse_sse_list.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    host.sat_parse_sse_list.restype = ctypes.c_int
    out = np.full(order + 1, 0xEE, np.uint8)                 # one byte past what the parser may write
    err = ctypes.create_string_buffer(128)
    m = host.sat_parse_sse_list(text.encode(), order, out.ctypes.data, err, len(err))
    assert out[order] == 0xEE
    if m < 0:
        assert m == -1 and err.value
        return None, err.value.decode()
    assert 1 <= m <= order
    return (out[:m].astype(int) + 1).tolist(), None


# ---------------------------------------------------------------- the parser
@pytest.mark.parametrize("text,order,want", [
    ("1", 8, [1]),
    ("2,1,8,5,3", 8, [2, 1, 8, 5, 3]),
    ("3-7", 8, [3, 4, 5, 6, 7]),
    ("1-3,9,5-6", 9, [1, 2, 3, 9, 5, 6]),
    ("1-8", 8, list(range(1, 9))),
    ("1-111", 111, list(range(1, 112))),
    ("1", 1, [1]),
])
def test_parser_accepts(text, order, want):
    assert parse(text, order) == (want, None)


@pytest.mark.parametrize("text,order,message", [
    ("0", 8, "SSE 0 out of range 1..8"),
    ("9", 8, "SSE 9 out of range 1..8"),
    ("3,3", 8, "SSE 3 twice"),
    ("2-4,3", 8, "SSE 3 twice"),
    ("5-2", 8, "range 5-2 descends"),
    ("1,,2", 8, "empty item"),
    ("1,", 8, "empty item"),
    ("-3", 8, "empty item"),
    ("1x", 8, "trailing text 'x'"),
    ("", 8, "empty item"),
    (",".join(str(v) for v in range(1, 113)), 111, "SSE 112 out of range 1..111"),
    (",".join(str(v) for v in list(range(1, 112)) + [5]), 111, "SSE 5 twice"),
])
def test_parser_refuses(text, order, message):
    assert parse(text, order) == (None, message)


def test_parser_under_the_sanitizers(tmp_path):
    """sat_parse.c and tests/native/motif_check.c - a stand-alone program with its own main that replays these lists
    against results written out in its source - built with -fsanitize=address,undefined and run as a child; no report may
    appear.  Nothing is loaded into Python, nothing is preloaded."""
    exe = str(tmp_path / "motif_check")
    build = subprocess.run(["gcc", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-Wall", "-Wextra", "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "motif_check.c"),
                            os.path.join(HOST, "sat_parse.c"), "-lpthread"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout == "motif_check: ok\n"
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr and p.stderr == ""


# ---------------------------------------------------------------- -c -q against a stand-alone -c query
# (entry, list) of the edge database, 0-based; None: the whole structure.  No sub-matrix holds a distance of 100 A or
# more (the entries that have such cells, 17 and 24, are not used), so the written query file reads back exactly.
MOTIFS = [
    (3, [4, 20, 50, 96, 70]),              # five SSEs of a 97-SSE entry, the last two out of order
    (6, list(range(2, 10))),               # ascending: a substructure of the 64-SSE entry
    (18, [1, 0, 7, 4, 2]),                 # permuted
    (0, [16]),                             # m = 1
    (25, None),                            # a whole structure between the motifs
    (18, list(range(8))),                  # the identity list
    (20, [100, 3, 99, 70, 2, 1]),          # a 101-SSE entry, cells with ? codes among them
]


def test_host_mode_motifs_equal_stand_alone_queries(golden_dir, tmp_path):
    db = sat.StructSet.read(os.path.join(golden_dir, ec.EDGE_DB))
    entries, lists = [e for e, _ in MOTIFS], [l for _, l in MOTIFS]
    subs = ml.dense_queries(db, entries, lists)
    assert all((d < 100.0).all() for _, d, _ in subs)
    assert [t.shape[0] for t, _, _ in subs] == [5, 8, 5, 1, 9, 8, 6]
    qset = sat.StructSet.from_dense([t.shape[0] for t, _, _ in subs], [t for t, _, _ in subs], [d for _, d, _ in subs],
                                    [db.names[e] for e in entries])
    qfile = tmp_path / "motifs.query"
    qset.write_ascii(qfile)
    back = sat.StructSet.read(qfile, "query")
    assert len(back) == len(subs)
    for s, (t, d, ty) in enumerate(subs):                      # what was written is what the motifs are
        bt, bd = back.dense(s)
        assert np.array_equal(bt, t) and bd.tobytes() == d.tobytes() and np.array_equal(back.ssetypes(s), ty)
    alone = run(golden_dir, ["-c", "-r", "16"], (ec.EDGE_DB + "\nT T F\n").encode() + open(qfile, "rb").read())
    assert alone.returncode == 0, alone.stderr[-400:]
    motif = run(golden_dir, ["-c", "-r", "16", "-q", ec.EDGE_DB], ml.stdin_lines(db, entries, lists))
    assert motif.returncode == 0, motif.stderr[-400:]
    lines = motif.stdout.split(b"\n")
    sses = [i for i, line in enumerate(lines) if line.startswith(b"# QUERY SSES = ")]
    # both classes' blocks of the six motifs carry the list, directly after # DBFILE, as given; the whole structure's do not
    want = [("# QUERY SSES = " + ml.spell(l)).encode() for l in lists if l is not None]
    assert [lines[i] for i in sses] == want + want
    assert all(lines[i - 1].startswith(b"# DBFILE = ") and lines[i - 2].startswith(b"# QUERY ID = ") for i in sses)
    assert motif.stdout.count(BLOCK) == 2 * len(MOTIFS)
    kept = b"\n".join(line for i, line in enumerate(lines) if i not in set(sses))
    # (the query file carries the entries' names, so the # QUERY ID lines are the same as they stand)
    assert kept == alone.stdout


def test_a_motif_line_leaves_the_earlier_blocks_alone(golden_dir):
    """the committed -c -q bytes with one motif line appended to the SID list.  The host mode draws from ONE random
    stream, class after class: the blocks before the motif's first one - the small class's of every listed SID - are
    the committed bytes; the motif's small-class block follows them; what comes later in the stream may differ."""
    name, bodies, _, restarts = [j for j in ec.EDGE_JOBS if j[1] is None][0]
    args, stdin = ec.job_command((name, bodies, None, restarts), golden_dir)
    want = open(os.path.join(ROOT, "tests", "golden", "expected", name + ".out"), "rb").read()
    nsid = len(ec.edge_sids()[0])
    p = run(golden_dir, ["-c"] + args, stdin + (ec.edge_name(18) + "@2,1,8,5,3\n").encode())
    assert p.returncode == 0, p.stderr[-400:]
    got_blocks, want_blocks = p.stdout.split(BLOCK), want.split(BLOCK)
    assert len(want_blocks) == 1 + 2 * nsid and len(got_blocks) == 1 + 2 * (nsid + 1)
    assert got_blocks[:1 + nsid] == want_blocks[:1 + nsid]
    assert b"# QUERY SSES" not in BLOCK.join(got_blocks[:1 + nsid])
    assert b"# QUERY ID = " + ec.edge_name(18).encode() in got_blocks[1 + nsid] and b"\n# QUERY SSES = 2,1,8,5,3\n" in got_blocks[1 + nsid]
    # and without the line: the committed bytes
    p = run(golden_dir, ["-c"] + args, stdin)
    assert p.returncode == 0 and p.stdout == want


# ---------------------------------------------------------------- refusals, usage, declarations
@pytest.mark.parametrize("line,message", [
    ("e18n008@2,1,9", b"ERROR: query e18n008@2,1,9: SSE 9 out of range 1..8\n"),
    ("e18n008@2,1,2", b"ERROR: query e18n008@2,1,2: SSE 2 twice\n"),
    ("e18n008@2,,1", b"ERROR: query e18n008@2,,1: empty item\n"),
    ("e18n008@", b"ERROR: query e18n008@: empty item\n"),
    ("e18n008@1-3 ", b"ERROR: query e18n008@1-3 : trailing text ' '\n"),
    ("nosuch1@1,2", b"ERROR: query nosuch1 not found\n"),
    # the text before '@' is longer than 7 characters: the cut comes after the split at '@', so the entry IS found and
    # its list checked (cut first, as on a line without '@', this would be "e18n008" with no list)
    ("e18n008x@2,1,9", b"ERROR: query e18n008@2,1,9: SSE 9 out of range 1..8\n"),
    ("e18n008@" + ",".join(["1"] * 1100), b"ERROR: query line with a list is longer than 2046 characters\n"),
])
@pytest.mark.parametrize("mode", [["-c", "-q"], ["-q"], ["-Q"]], ids=["c-q", "q", "Q"])
def test_cli_refusals(golden_dir, mode, line, message):
    """a bad list ends the run when the database is read, before any search and before a GPU is touched: exit 1, one
    ERROR line, nothing on stdout, no search's or device's banner.  (The "MAXDIM = 111" line is not asked about: main()
    prints it before it reads stdin, in every run and for the existing "not found" error too, so it cannot go without
    changing what runs without a motif print.)"""
    stdin = (ec.edge_name(6) + "\n" + line + "\n" + ec.edge_name(3) + "\n").encode()
    p = run(golden_dir, ["-r", "16"] + mode + [ec.EDGE_DB], stdin)
    assert p.returncode == 1, p.stderr
    assert message in p.stderr, p.stderr
    assert p.stderr.count(b"ERROR:") == 1 and p.stdout == b""
    assert b"Executing" not in p.stderr and b"HIP device" not in p.stderr and b"maxstart" not in p.stderr


def test_a_long_sid_and_a_crlf_line_name_the_same_motif(golden_dir):
    """what stands before '@' is cut to 7 characters after the split, and a carriage return before the line's end is no
    part of the list: both lines are the motif of the plain one"""
    plain = run(golden_dir, ["-c", "-r", "16", "-q", ec.EDGE_DB], (ec.edge_name(18) + "@2,1,8,5,3\n").encode())
    assert plain.returncode == 0 and plain.stdout.count(b"\n# QUERY SSES = 2,1,8,5,3\n") == 2, plain.stderr[-400:]
    for line in (ec.edge_name(18) + "x@2,1,8,5,3\n", ec.edge_name(18) + "@2,1,8,5,3\r\n", ec.edge_name(18) + "@2,1,8,5,3"):
        p = run(golden_dir, ["-c", "-r", "16", "-q", ec.EDGE_DB], line.encode())
        assert p.returncode == 0 and p.stdout == plain.stdout, (line, p.stderr[-400:])


def test_usage_names_the_syntax(golden_dir):
    p = run(golden_dir, ["-x"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"  SID@list : (-q, -Q) a stdin line may name a motif" in p.stderr and b"d1ubia_@2,1,8,5,3" in p.stderr
    assert b"[-q dbfile | -Q dbfile | -a dbfile]" in p.stderr
    assert b"  -Q dbfile : as -q dbfile" in p.stderr and b"  -a dbfile : all-vs-all" in p.stderr


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "satabsearch.h")).read()
    text = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    for decl in ("int sat_queries_from_db_sses(sat_ctx *ctx, int n_queries, const int32_t *entry, const int32_t *sse_begin, "
                 "const uint8_t *sse, uint32_t first_query_ordinal);",
                 "int sat_multi_queries_from_db_sses(sat_multi *m, int n_queries, const int32_t *entry, const int32_t *sse_begin, "
                 "const uint8_t *sse, uint32_t first_query_ordinal);"):
        assert decl in text, decl
        assert decl[4:decl.index("(")] in _native.ABI_SYMBOLS
    assert "#define SAT_ABI_VERSION 1" in text
    parse_h = open(os.path.join(HOST, "sat_parse.h")).read()
    assert "int sat_parse_sse_list(const char *text, int order, uint8_t *out, char *err, size_t err_len);" in parse_h


def test_python_packs_the_lists():
    from cuda_satabsearch_amd.search import _pack_sse_lists
    begin, sse = _pack_sse_lists([[2, 1], None, [], (5,)], 4)
    assert begin.dtype == np.int32 and begin.tolist() == [0, 2, 2, 2, 3] and sse.dtype == np.uint8 and sse.tolist() == [2, 1, 5]
    begin, sse = _pack_sse_lists([None], 1)
    assert begin.tolist() == [0, 0] and sse.size >= 1
    with pytest.raises(ValueError):
        _pack_sse_lists([[1]], 2)
    with pytest.raises(ValueError):
        _pack_sse_lists([[256]], 1)
