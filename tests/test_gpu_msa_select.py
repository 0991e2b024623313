"""GPU: sw_msa_select (state, residues, counts, depth, rows, levels) against tests/msa_select_ref.py on inputs built directly
in numpy, against sw_msa_filter itself at D = 0, then the host driver and `align --outMsa` with the selection flags."""
import numpy as np
import pytest

import gpu_util as G
import msa_ref as M
import msa_select_ref as R
from test_gpu_msa import TOP, host_arrays, letters_of, run_align, small_db  # noqa: F401  (the small family DB and its helpers)

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def env():
    torch, capi, _ = G.gpu_modules()
    ctx = capi.Context(0)
    yield torch, capi, ctx
    ctx.close()


def upload(torch, case, include=None, with_query=True):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = case["n"]
    hold = dict(q=dev(case["query"]) if with_query else None)
    if n:
        hold.update(ch=dev(case["chars"]), off=dev(case["offsets"].view(np.int64)), len=dev(case["lengths"]),
                    res=dev(np.frombuffer(case["results"].tobytes(), dtype=np.uint8).copy()), cig=dev(case["cigar"].view(np.int32)))
    hold["inc"] = dev(np.ascontiguousarray(include, dtype=np.uint8)) if include is not None else None
    ptr = lambda k: hold[k].data_ptr() if hold.get(k) is not None else 0
    args = dict(query=ptr("q"), qlen=case["qlen"], n=n, chars=ptr("ch"), offsets=ptr("off"), lengths=ptr("len"), results=ptr("res"),
                cigar=ptr("cig"), include=ptr("inc"))
    return hold, args


def run_select(env, case, C=0, Q=0, D=0, ladder=(90,), include=None, with_query=True, optional=True, uploaded=None):
    """sw_msa_select on the case's arrays.  Every output starts as garbage and sits between guard bytes, which must survive."""
    torch, capi, ctx = env
    n, qlen = case["n"], case["qlen"]
    assert capi.align_result_dtype() == M.RECORD
    hold, args = uploaded or upload(torch, case, include, with_query)
    sizes = dict(state=n + 1, residues=4 * (n + 1), counts=16)
    if optional:
        sizes.update(depth=4 * qlen, rows=(n + 1) * qlen, levels=(n + 1) * (n + 1))
    bufs = {k: torch.full((GUARD + v + GUARD,), 0xA7, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    args = dict(args, min_coverage=C, min_query_identity=Q, diff=D, ladder=ladder,
                **{k: b.data_ptr() + GUARD for k, b in bufs.items()})
    need = capi.msa_select(ctx, **args)
    assert need > 0
    temp = torch.full((need,), 0xEE, dtype=torch.uint8, device="cuda")
    assert capi.msa_select(ctx, temp=temp.data_ptr(), temp_bytes=need, **args) == need
    torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        raw = b.cpu().numpy()
        assert (raw[:GUARD] == 0xA7).all() and (raw[-GUARD:] == 0xA7).all(), k
        out[k] = raw[GUARD:-GUARD].copy()
    out["residues"] = out["residues"].view(np.int32)
    out["counts"] = out["counts"].view(np.int32).tolist()
    if optional:
        out["depth"] = out["depth"].view(np.int32)
        out["rows"] = out["rows"].reshape(n + 1, qlen)
        out["levels"] = out["levels"].reshape(n + 1, n + 1)
    return out


def reference(case, C=0, Q=0, D=0, ladder=(90,), include=None, with_query=True, trace=None):
    rows = R.case_rows(case, include, with_query)
    idents = R.ident_matrix(rows)
    state, depth, counts = R.select(rows, C, Q, D, ladder, trace=trace, idents=idents)
    return dict(rows=rows, residues=M.residues(rows), state=state, depth=depth, counts=counts, levels=R.levels(rows, ladder, idents))


def assert_equal(got, want):
    if "rows" in got:
        assert got["rows"].tobytes() == want["rows"].tobytes(), np.argwhere(got["rows"] != want["rows"])[:5]
        assert got["levels"].tobytes() == want["levels"].tobytes(), np.argwhere(got["levels"] != want["levels"])[:5]
    assert got["residues"].tolist() == want["residues"].tolist()
    assert got["state"].tolist() == want["state"].tolist(), np.flatnonzero(got["state"] != want["state"])[:10]
    if "depth" in got:
        assert got["depth"].tolist() == want["depth"].tolist()
    assert got["counts"] == want["counts"]


LADDERS = [(90,), (50, 94), (20, 40, 60, 80, 95), tuple(range(10, 90, 5))]
NS = [0, 1, 63, 64, 65, 130, 200]


@pytest.mark.parametrize("qlen", [1, 31, 32, 33, 63, 64, 65, 127, 129, 700])
def test_shapes_against_reference(env, qlen):
    """every qlen of the list against every n of the list; D, the ladder, C, Q, the include bytes and the master rotate, and
    over the ten qlen every n meets every D and every ladder length"""
    assert [len(l) for l in LADDERS] == [1, 2, 5, 16]
    rng = np.random.default_rng(3000 + qlen)
    at = [1, 31, 32, 33, 63, 64, 65, 127, 129, 700].index(qlen)
    for k, n in enumerate(NS):
        case = M.random_case(rng, qlen, n, max_runs=12 if qlen < 700 else 40, families=3, copy_rate=0.1)
        D = [0, 1, 3, n + 1][(k + at) % 4]
        ladder = LADDERS[(k + at // 4 + at) % 4]
        with_query = (k + at) % 3 != 2
        C = [0, 30][(k + at) % 2]
        Q = [0, 5, 0][(k + at) % 3] if with_query else 0
        include = (rng.random(n) < 0.8).astype(np.uint8) if k % 2 else None
        got = run_select(env, case, C, Q, D, ladder, include, with_query)
        want = reference(case, C, Q, D, ladder, include, with_query)
        assert_equal(got, want)
        if n >= 63:
            assert (want["rows"][:n] == 20).any() or qlen == 1
            assert (case["results"]["status"] != 0).any() and (case["results"]["cigar_len"] == 0).any()
        if not with_query:
            assert (got["rows"][n] == M.NONE).all() and got["state"][n] == 0


@pytest.mark.parametrize("D", ["0", "1", "3", "n+1"])
@pytest.mark.parametrize("ladder", LADDERS, ids=lambda l: "T%d" % len(l))
def test_every_depth_and_ladder(env, D, ladder):
    """every D of the list with every ladder length, over three blocks of rows and five words of columns"""
    n, qlen = 130, 129
    case = M.random_case(np.random.default_rng(len(ladder) * 7 + len(D)), qlen, n, families=4, copy_rate=0.12)
    d = n + 1 if D == "n+1" else int(D)
    trace = []
    want = reference(case, 0, 0, d, ladder, trace=trace)
    assert_equal(run_select(env, case, 0, 0, d, ladder), want)
    lean = run_select(env, case, 0, 0, d, ladder, optional=False)   # the optional outputs are optional
    assert lean["state"].tolist() == want["state"].tolist() and lean["counts"] == want["counts"]
    if len(ladder) > 1 and d != 1:   # (D = 1: the first rung's rows put a residue into every column, nobody is needed after it)
        assert len({t for t, _ in trace}) > 1


def test_guard_case_set(env):
    """the cases of the CPU guard (test_msa_select_cpu.py): every state, several rungs, keeps behind lower-ranked rows"""
    for qlen, n, f in R.GUARD_CASES:
        for seed in R.GUARD_SEEDS:
            case = R.guard_case(qlen, n, f, seed)
            p = R.GUARD_PARAMS
            got = run_select(env, case, p["C"], p["Q"], p["D"], p["ladder"])
            assert_equal(got, reference(case, p["C"], p["Q"], p["D"], p["ladder"]))


def planted(qlen, rows_codes, master):
    """hits whose rows are given (codes 0 .. 20, M.NONE: not aligned there): one '=' run per stretch of aligned positions"""
    n = len(rows_codes)
    recs = np.zeros(n, dtype=M.RECORD)
    subjects, words, at = [], [], 0
    for h, codes in enumerate(rows_codes):
        codes = np.asarray(codes)
        on = np.flatnonzero(codes != M.NONE)
        lo, hi = int(on[0]), int(on[-1]) + 1
        assert (codes[lo:hi] != M.NONE).all()
        subjects.append(codes[lo:hi].astype(np.int8))
        recs[h]["q_begin"], recs[h]["q_end"], recs[h]["s_end"] = lo, hi, hi - lo
        recs[h]["cigar_len"], recs[h]["cigar_offset"] = 1, at
        words.append((hi - lo) << 4 | M.OP_EQ)
        at += 1
    lengths = np.array([len(s) for s in subjects], dtype=np.int32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    return dict(query=np.asarray(master, dtype=np.int8), qlen=qlen, n=n, chars=np.concatenate(subjects + [np.zeros(4, np.int8)]),
                offsets=offsets, lengths=lengths, results=recs, cigar=np.array(words + [0], dtype=np.uint32))


def test_worked_example(env):
    b = np.array([1] * 10 + [0, 0, 0, 0, 2, 2, 2, 2, 2, 2])
    a = b.copy()
    a[:10] = M.NONE
    case = planted(20, [a, b], np.zeros(20))
    got = run_select(env, case, D=10, ladder=(40, 100))
    assert got["state"].tolist() == [4, 1, 1] and got["depth"].tolist() == [2] * 20 and got["counts"] == [1, 0, 0, 1]
    assert got["levels"].tolist() == [[0, 2, 1], [1, 0, 0], [0, 0, 0]]
    assert_equal(got, reference(case, D=10, ladder=(40, 100)))
    got = run_select(env, case, D=10, ladder=(100,))
    assert got["state"].tolist() == [1, 1, 1] and got["depth"].tolist() == [2] * 10 + [3] * 10 and got["counts"] == [2, 0, 0, 0]
    assert run_select(env, case, C=60, ladder=(100,))["state"].tolist() == [2, 1, 1]
    assert run_select(env, case, Q=30, ladder=(100,))["state"].tolist() == [1, 3, 1]


@pytest.mark.parametrize("P", [1, 50, 94, 100])
def test_no_diff_is_the_greedy_filter(env, P):
    """D = 0, C = Q = 0 and the ladder {P}: state == 1 is `keep` of sw_msa_filter, run on the same device buffers"""
    torch, capi, ctx = env
    case = M.random_case(np.random.default_rng(40 + P), 129, 200, families=4, copy_rate=0.08)
    include = (np.random.default_rng(P).random(200) < 0.9).astype(np.uint8)
    hold, args = upload(torch, case, include)
    got = run_select(env, case, ladder=(P,), optional=False, uploaded=(hold, args))
    n = case["n"]
    dres = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    dkeep = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    dpurged = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = dict(max_identity=P, residues=dres.data_ptr(), keep=dkeep.data_ptr(), purged=dpurged.data_ptr())
    need = capi.msa_filter(ctx, **args, **out)
    temp = torch.zeros(need, dtype=torch.uint8, device="cuda")
    capi.msa_filter(ctx, temp=temp.data_ptr(), temp_bytes=need, **args, **out)
    torch.cuda.synchronize()
    keep = dkeep.cpu().numpy()
    assert (got["state"] == 1).astype(int).tolist() == keep.tolist() and 0 < keep.sum() <= n
    assert got["residues"].tolist() == dres.cpu().numpy().tolist()
    assert got["counts"] == [int(keep[:n].sum()), 0, 0, int(dpurged.item())]
    assert set(got["state"].tolist()) <= {0, 1, 4}


@pytest.mark.parametrize("D", [0, 1, 3, 301])
def test_copies_are_thinned(env, D):
    one = np.random.default_rng(5).integers(0, 20, 90)
    case = planted(90, [one] * 300, np.full(90, 20))     # (the master is all 'X': no residue)
    got = run_select(env, case, D=D, ladder=(20, 94), optional=False)
    assert got["state"].tolist() == [1] + [4] * 299 + [0] and got["counts"] == [1, 0, 0, 299]


def test_several_tiles(env):
    """n = 600, qlen = 700: ten tiles of 64 rows (three workgroups of the levels kernel per tile row), 22 words; the
    reference's identity counts come from one-hot matrix products"""
    case = M.random_case(np.random.default_rng(2025), 700, 600, max_runs=30, families=8, copy_rate=0.1, no_part_rate=0.05)
    rows = R.case_rows(case)
    n = case["n"]
    half = M.pair_ident_onehot(rows).astype(np.int64)
    idents = half + half.T
    assert idents[5, 3] == M.ident(rows[3], rows[5]) == idents[3, 5] and idents[n, 7] == M.ident(rows[n], rows[7])
    ladder = (20, 40, 60, 80, 95)
    for D in (0, 5):
        got = run_select(env, case, 20, 5, D, ladder)
        state, depth, counts = R.select(rows, 20, 5, D, ladder, idents=idents)
        assert got["levels"].tobytes() == R.levels(rows, ladder, idents).tobytes()
        assert got["state"].tolist() == state.tolist() and got["depth"].tolist() == depth.tolist() and got["counts"] == counts
        assert counts[0] > 8 and (D == 0 or counts[3] > 50)


def test_temp_contract_and_argument_checks(env):
    torch, capi, ctx = env
    buf = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    b = buf.data_ptr()
    ok = dict(query=b, qlen=10, n=0, chars=0, offsets=0, lengths=0, results=0, cigar=0, include=0, min_coverage=50,
              min_query_identity=20, diff=3, ladder=(30, 60, 90), state=b + 64, residues=b + 128, counts=b + 192)
    need = capi.msa_select(ctx, **ok)            # temp == NULL: reports, launches nothing
    assert need > 0 and int(buf.sum().item()) == 0
    # the need depends on qlen, n, the number of rungs and the optional outputs, not on the thresholds
    assert capi.msa_select(ctx, **dict(ok, min_coverage=0, min_query_identity=0, diff=0, ladder=(1, 2, 3))) == need
    assert capi.msa_select(ctx, **dict(ok, ladder=tuple(range(1, 17)))) >= need
    assert capi.msa_select(ctx, **dict(ok, qlen=5000)) > need
    assert capi.msa_select(ctx, **dict(ok, n=500, chars=b, offsets=b, lengths=b, results=b, cigar=b)) > need
    with pytest.raises(capi.SwError) as e:
        capi.msa_select(ctx, temp=b + 4096, temp_bytes=need - 1, **ok)
    assert e.value.code == -5
    assert int(buf.sum().item()) == 0
    capi.msa_select(ctx, temp=b + 4096, temp_bytes=need, **ok)
    torch.cuda.synchronize()
    for bad in (dict(qlen=0), dict(qlen=(1 << 22) + 1), dict(n=-1), dict(n=(1 << 14) + 1), dict(min_coverage=-1),
                dict(min_coverage=101), dict(min_query_identity=-1), dict(min_query_identity=101), dict(query=0), dict(diff=-1),
                dict(ladder=()), dict(ladder=None), dict(ladder=tuple(range(1, 18))), dict(ladder=(0, 50)), dict(ladder=(50, 101)),
                dict(ladder=(50, 50)), dict(ladder=(60, 50)), dict(residues=0), dict(state=0), dict(counts=0), dict(n=2),
                dict(n=2, chars=b, offsets=b, lengths=b, results=b)):
        before = buf.clone()
        with pytest.raises(capi.SwError) as e:
            capi.msa_select(ctx, temp=b + 4096, temp_bytes=1 << 18, **dict(ok, **bad))
        assert e.value.code == -1, bad
        torch.cuda.synchronize()
        assert bool((buf == before).all()), bad    # nothing was launched
    assert capi.msa_select(ctx, **dict(ok, query=0, min_query_identity=0)) == need   # no master is fine without Q


# ---- the host driver and the command line -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def family(small_db):
    """the small family DB of test_gpu_msa.py, scanned and aligned once: the reference's rows and identity counts"""
    from cudasw4_amd import driver
    db = small_db
    d = driver.Driver(devices=[0], num_top=TOP)
    d.open_db(db["prefix"])
    result = d.scan(db["letters"])
    ids = result["ids"]
    subjects = [db["seqs"][int(d.reference_header(int(i)).split()[0][1:])] for i in ids]
    res, cigar_text = d.align_hits(db["letters"], result)
    chars, offsets, lengths, rec, cig = host_arrays(subjects, ids, res, cigar_text)
    rows = M.build_rows(db["q"], len(db["q"]), chars, offsets, lengths, rec, cig)
    yield dict(db=db, d=d, result=result, rows=rows, idents=R.ident_matrix(rows), n=len(ids))
    d.close()


DEFAULT_LADDER = (20, 30, 40, 50, 60, 70, 80, 90)
VARIANTS = [
    (dict(min_coverage=70), ["--msaMinCoverage", "70"], dict(C=70, ladder=(100,))),
    (dict(min_query_identity=60), ["--msaMinQueryIdentity", "60"], dict(Q=60, ladder=(100,))),
    (dict(diff=2), ["--msaDiff", "2"], dict(D=2, ladder=DEFAULT_LADDER)),
    (dict(diff=3, ladder=(30, 60, 95)), ["--msaDiff", "3", "--msaDiffLadder", "30,60,95"], dict(D=3, ladder=(30, 60, 95))),
]


@pytest.mark.parametrize("kw,flags,ref", VARIANTS, ids=[v[1][0][2:] + ("Ladder" if len(v[1]) > 2 else "") for v in VARIANTS])
def test_driver_and_command_line(family, kw, flags, ref):
    """Driver.hit_msa with each new argument against the reference on Driver.align_hits' output, and `align --outMsa` with the
    flag against Driver.hit_msa: the file and the --verbose line"""
    db, d, n = family["db"], family["d"], family["n"]
    want_state, want_depth, want_counts = R.select(family["rows"], idents=family["idents"], **ref)
    got = d.hit_msa(db["letters"], family["result"], query_header="query one", **kw)
    assert got["rows"].tobytes() == family["rows"].tobytes()
    assert got["state"].tolist() == want_state.tolist() and got["depth"].tolist() == want_depth.tolist()
    assert got["counts"] == want_counts and got["ladder"] == list(ref["ladder"])
    assert got["keep"].tolist() == (want_state == 1).astype(int).tolist() and got["purged"] == want_counts[3]
    kept = [k for k in range(n) if want_state[k] == 1]
    lines = got["a3m"].splitlines()
    assert lines[0] == ">query one" and len(lines) == 2 + 2 * len(kept) and 0 < len(kept) < int((want_state[:n] != 0).sum())
    assert [l[1:] for l in lines[2::2]] == [d.reference_header(int(family["result"]["ids"][k])) for k in kept]
    assert want_counts[{"C": 1, "Q": 2, "D": 3}[sorted(ref)[0]]] > 0    # the flag under test left something out
    prefix = str(db["tmp"] / ("S" + flags[0][2:] + str(len(flags))))
    _, stdout = run_align(db, ["--outMsa", prefix, "--verbose"] + flags, str(db["tmp"] / "s.txt"))
    assert open(prefix + ".0.a3m").read() == got["a3m"]
    assert "msa: %d of %d results written, %d below coverage, %d below query identity, %d thinned, 0 without a trace\n" % (
        len(kept), TOP, want_counts[1], want_counts[2], want_counts[3]) in stdout


def test_ladder_defaults_of_the_driver(family):
    """the rungs Driver.hit_msa takes: {max_identity} without diff, 20, 30, ... up to max_identity (default 90) with it"""
    db, d = family["db"], family["d"]
    for kw, ref in ((dict(min_coverage=50, max_identity=90), dict(C=50, ladder=(90,))),
                    (dict(diff=3, max_identity=45), dict(D=3, ladder=(20, 30, 40, 45))),
                    (dict(diff=1000, min_coverage=30, min_query_identity=20), dict(D=1000, C=30, Q=20, ladder=DEFAULT_LADDER))):
        got = d.hit_msa(db["letters"], family["result"], **kw)
        want = R.select(family["rows"], idents=family["idents"], **ref)
        assert got["ladder"] == list(ref["ladder"]) and got["state"].tolist() == want[0].tolist() and got["counts"] == want[2]
    with pytest.raises(ValueError):
        d.hit_msa(db["letters"], family["result"], diff=2, ladder=(30, 60), max_identity=90)
    with pytest.raises(ValueError):
        d.hit_msa(db["letters"], family["result"], diff=0)
    with pytest.raises(ValueError):
        d.hit_msa(db["letters"], family["result"], min_coverage=101)


def test_without_the_new_flags_the_files_are_the_filters(family):
    """--outMsa alone and with --msaMaxIdentity 90 write what Driver.hit_msa(max_identity=...) gives through sw_msa_filter,
    with today's --verbose line"""
    db, d = family["db"], family["d"]
    for flags, P in (([], None), (["--msaMaxIdentity", "90"], 90)):
        want = d.hit_msa(db["letters"], family["result"], max_identity=P, query_header="query one")
        assert "state" not in want
        prefix = str(db["tmp"] / ("K%d" % len(flags)))
        _, stdout = run_align(db, ["--outMsa", prefix, "--verbose"] + flags, str(db["tmp"] / "k.txt"))
        assert open(prefix + ".0.a3m").read() == want["a3m"]
        assert "msa: %d of %d results written, %d purged, 0 without a trace\n" % (int(want["keep"][:family["n"]].sum()), TOP,
                                                                                   want["purged"]) in stdout
        assert "below coverage" not in stdout and "thinned" not in stdout
