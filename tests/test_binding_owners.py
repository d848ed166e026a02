"""The one owner type of the ctypes binding (kompass_hip._Owner) and its explicit loader (kompass_hip.load).

Without a GPU: the eight owner classes share close / __del__ / __enter__ / __exit__ by identity, and load() of a
shared object that exports none of the library's symbols -- the C library -- either fails naming a symbol or, with
tolerant=True, binds stubs that name the symbol and the path when they are called.

On the GPU: `with` and close() on each of the seven device contexts, the exception a call after close() raises, and
timings() of the four contexts that have it against the kernel names the commit before this one returned for the
same calls."""
import ctypes.util
import subprocess
import sys
import textwrap

import pytest

import kompass_hip as kh
import synthetic as syn
import test_context_lifecycle as lifecycle

OWNERS = (kh.Comm, kh.DwaContext, kh.MapperContext, kh.CloudContext, kh.ZoneContext, kh.DepthContext, kh.DvzContext,
          kh.PlannerContext)
LIBC = ctypes.util.find_library("c")


@pytest.mark.parametrize("member", ["close", "__del__", "__enter__", "__exit__"])
def test_owner_members_are_the_base_class_functions(member):
    base = getattr(kh._Owner, member)
    assert callable(base)
    for cls in OWNERS:
        assert issubclass(cls, kh._Owner)
        assert getattr(cls, member) is base, f"{cls.__name__}.{member}"
        assert member not in vars(cls)


def test_timing_and_stream_members_are_shared():
    timed = (kh.DwaContext, kh.MapperContext, kh.CloudContext, kh.DepthContext)
    ordered = (kh.CloudContext, kh.DepthContext, kh.PlannerContext)
    for member, classes in (("timing_enable", timed), ("timings", timed), ("after_stream", ordered)):
        assert len({getattr(cls, member) for cls in classes}) == 1, member
        for cls in set(OWNERS) - set(classes):
            assert not hasattr(cls, member), f"{cls.__name__}.{member}"
    assert [cls._timing_cap for cls in timed] == [32, 16, 16, 16]
    assert [cls._kc for cls in OWNERS] == ["kc_comm", "kc_dwa", "kc_mapper", "kc_cloud", "kc_zone", "kc_depth", "kc_dvz",
                                           "kc_planner"]


def test_close_without_a_handle_is_harmless():
    """An owner whose constructor failed before the handle existed, and one whose handle is null."""
    for cls in OWNERS:
        ctx = cls.__new__(cls)
        ctx.close()
        ctx.h = kh._vp()
        with ctx as same:
            assert same is ctx
        assert not ctx.h.value


def _run(body):
    """`body` in a fresh interpreter (the test session's loaded library stays what it is); -> its stdout."""
    code = "import sys\nsys.path[:0] = %r\nimport kompass_hip as kh\nLIBC = %r\n" % (sys.path, LIBC) + textwrap.dedent(body)
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    return done.stdout


def test_tolerant_load_binds_stubs_that_name_symbol_and_path():
    assert LIBC, "no C library found"
    out = _run("""
        L = kh.load(LIBC, tolerant=True)
        assert kh.lib() is L
        assert all(callable(getattr(L, name)) for name in kh.SIGNATURES)
        assert sorted(kh._fast) == sorted(kh._fast_protos()) and all(callable(f) for f in kh._fast.values())
        for call in (L.kc_abi_version, kh._fast["kc_dwa_cycle"], lambda: kh.DwaContext(kh.CYLINDER, [0.1, 0.4])):
            try:
                call()
            except kh.KompassHipError as e:
                print(e)
            else:
                raise SystemExit("the stub returned")
        """).splitlines()
    assert len(out) == 3
    for line, symbol in zip(out, ("kc_abi_version", "kc_dwa_cycle", "kc_dwa_create")):
        assert symbol in line and LIBC in line, line


def test_strict_load_fails_and_names_a_missing_symbol():
    assert LIBC, "no C library found"
    out = _run("""
        try:
            kh.load(LIBC)
        except kh.KompassHipError as e:
            print(e)
        else:
            raise SystemExit("the load succeeded")
        assert kh._lib is None and not kh._fast
        """)
    assert any(name in out for name in kh.SIGNATURES) and LIBC in out, out


def test_load_of_a_missing_file_says_how_to_build(tmp_path):
    out = _run(f"""
        try:
            kh.load({str(tmp_path / "libkompass_hip.so")!r})
        except kh.KompassHipError as e:
            print(e)
        """)
    assert "is missing: build it with" in out


# ---- on the GPU --------------------------------------------------------------------------------------------------
# What a call after close() raised at the commit before this one: the library's refusal of a null context.
AFTER_CLOSE = {"dwa": ValueError, "mapper": ValueError, "cloud": ValueError, "zone": ValueError, "depth": ValueError,
               "dvz": ValueError, "planner": ValueError}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(lifecycle.CONTEXTS))
def test_with_closes_and_a_closed_context_refuses(name):
    make, use = lifecycle.CONTEXTS[name]
    with make() as ctx:
        assert isinstance(ctx, kh._Owner) and ctx.h.value
    assert not ctx.h.value
    ctx.close()
    ctx.close()
    assert not ctx.h.value
    with pytest.raises(Exception) as err:
        use(ctx)
    assert type(err.value) is AFTER_CLOSE[name], repr(err.value)
    assert "null" in str(err.value)
    ctx.close()


ANGLES16, RANGES16 = syn.dense_scan(16, 0.2)
TIMED = {  # the smallest compute call of each context that has timings()
    "dwa": (lifecycle.make_dwa, lifecycle.use_dwa),
    "mapper": (lambda: kh.MapperContext(16, 16, 0.1, (0, 0, 0), 0.0, 16), lambda c: c.scan_to_grid(ANGLES16, RANGES16)),
    "cloud": (lifecycle.make_cloud, lifecycle.use_cloud),
    "depth": (lifecycle.make_depth, lifecycle.use_depth),
}
# the kernel names timings() returned for these calls at the commit before this one, recorded from a run of that
# commit's binding on an MI355X
PARENT_NAMES = {
    "dwa": ["segment_near_kernel", "cycle_kernel", "rollout_collide_kernel", "host:launch_rollout", "host:launch_collision", "host:wait_result", "host:launch_rollout", "host:launch_collision"],
    "mapper": ["grid_clear", "rays_kernel", "endpoints_kernel"],
    "cloud": ["cloud_extent_kernel", "cloud_grid_clear", "cloud_grid_scatter_kernel", "cloud_grid_decode_kernel", "host:cloud_grid_upload"],
    "depth": ["upload", "depth_boxes_kernel", "host:depth_stats"],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TIMED))
def test_timings_names_are_the_parents(name):
    make, use = TIMED[name]
    with make() as ctx:
        ctx.timing_enable(True)
        use(ctx)
        got = ctx.timings()
    assert got and all(type(n) is str and type(ms) is float for n, ms in got)
    assert [n for n, _ in got] == PARENT_NAMES[name]
