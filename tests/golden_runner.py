"""The product's whole host program in a process of its own over the oracle engine, for the runs that write the golden path
behind the silver paths (--golden_path, tests/test_golden_path_cpu.py).  It is the runner of tests/resident_runner.py with
the second engine table filled to its end: grp_reads_gather and grp_rewind restated over the oracle engine's batches (lists
of strings) and its filter.  GOLDEN_NO_ENTRIES: the two entries stay NULL (an engine without them); GOLDEN_GATHER_NOMEM=<n>:
the n-th gather and every later one says GRP_ERR_NOMEM; GOLDEN_OUT: a JSON file with the calls the two entries took."""
import resident_runner as RR

_EXTRA = '''
slice_dtype = np.dtype([("src", "<u4"), ("read", "<u4"), ("first_base", "<u4"), ("n_bases", "<u4")])
g_calls = {"gather": 0, "gather_slices": 0, "gather_sources": 0, "rewind": 0, "creates": 0}
_create = dict(host.VT_TYPES)["create"](C.cast(eng.vt.create, C.c_void_p).value)

def counted_create(params_p, out_pp):
    g_calls["creates"] += 1
    return _create(params_p, out_pp)

def reads_gather(ctx, srcs_p, n_srcs, slices_p, n_slices, out_pp):
    g_calls["gather"] += 1
    nomem = int(os.environ.get("GOLDEN_GATHER_NOMEM", "0"))
    if nomem and g_calls["gather"] >= nomem:
        return native.GRP_ERR_NOMEM
    srcs = C.cast(srcs_p, C.POINTER(C.c_void_p))
    sl = np.frombuffer(C.string_at(slices_p, n_slices * slice_dtype.itemsize), dtype=slice_dtype) if n_slices else []
    reads = []
    for s in sl:
        if int(s["src"]) >= n_srcs:
            return native.GRP_ERR_INVALID
        batch = eng.batches[srcs[int(s["src"])]]
        r = batch[int(s["read"])]
        f, n = int(s["first_base"]), int(s["n_bases"])
        if n < 1 or f + n > len(r):
            return native.GRP_ERR_INVALID
        reads.append(r[f:f + n])
    hnd = eng._next
    eng._next += 1
    eng.batches[hnd] = reads
    out_pp[0] = hnd
    g_calls["gather_slices"] += n_slices
    g_calls["gather_sources"] += n_srcs
    return 0

def rewind(ctx):
    g_calls["rewind"] += 1
    c = eng.ctx
    c["mf"] = orc.MiBF(c["m"], c["seeds"], c["tile"], c["k"])
    return 0

keep3 = [host.READS_GATHER_FN(reads_gather), host.REWIND_FN(rewind), dict(host.VT_TYPES)["create"](counted_create)]
eng.vt.create = keep3[2]
if not os.environ.get("GOLDEN_NO_ENTRIES"):
    ext.reads_gather, ext.rewind = keep3[0], keep3[1]
'''

_TAIL = '''
if os.environ.get("GOLDEN_OUT"):
    json.dump(g_calls, open(os.environ["GOLDEN_OUT"], "w"))
'''

_MAIN = RR._MAIN
assert RR.RUNNER.count(_MAIN) == 1 and RR.RUNNER.count("\nos._exit(rc)\n") == 1
# (RR.RUNNER is a format string: the braces of what is put into it are doubled)
RUNNER = RR.RUNNER.replace(_MAIN, _EXTRA.replace("{", "{{").replace("}", "}}") + _MAIN).replace("\nos._exit(rc)\n", _TAIL.replace("{", "{{").replace("}", "}}") + "\nos._exit(rc)\n")
