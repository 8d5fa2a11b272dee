"""Which argument check wins when a call carries two faults (csrc/stage2_api.cpp: the order of the checks is part of the
ABI).  For each of the seven window calls, on one tiny window, three calls with two faults each:

  1. a null token array and n = 1 << 31            -> MSJ_ERR_BAD_ARGUMENT (missing arrays are judged before the size)
  2. n = 1 << 31 and a misaligned d_idx            -> MSJ_CAPACITY         (the size is judged before the alignment)
  3. a null output whose capacity is above 0 and
     a misaligned d_depth                          -> MSJ_ERR_BAD_ARGUMENT

Nothing is launched by any of them: every output and result keeps its fill.  (msj_validate_device has no output with a
capacity: its third call leaves out d_result, its only output.)
"""
import pytest

from tests import test_validate_documents as tvd

pytestmark = pytest.mark.gpu

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
TOO_MANY = 1 << 31
WINDOW = b'{"a":[1,2]} "s" 3 '

# every call's arguments behind ctx, by name, and the output its third call leaves out
TOKENS = ("buf", "len", "idx", "n", "type", "depth", "match", "end", "flags")
SPLIT = ("first", "docs")
NUMBERS = ("numbers", "ncap", "nres")
CALLS = {
    "msj_validate_device": (TOKENS + ("nres", "max_depth", "res"), "res"),
    "msj_validate_documents_device": (TOKENS + SPLIT + NUMBERS + ("max_depth", "out0", "cap", "res"), "out0"),
    "msj_tape_device": (TOKENS + NUMBERS + ("aux0", "out0", "cap", "out1", "cap", "res"), "out0"),
    "msj_tape_documents_device": (TOKENS + SPLIT + NUMBERS + ("aux0", "out0", "cap", "out1", "cap", "out2", "cap", "res"), "out2"),
    "msj_select_documents_device": (("paths",) + TOKENS + SPLIT + NUMBERS + ("aux0", "out0", "cap", "res"), "out0"),
    "msj_array_column_device": (TOKENS[2:] + SPLIT + NUMBERS + ("aux0", "aux1", "out0", "out1", "cap", "out2", "cap", "res", "out3"), "out2"),
    "msj_select_elements_device": (("paths",) + TOKENS + NUMBERS + ("aux0", "aux1", "out0", "cap", "res"), "out0"),
}


@pytest.fixture(scope="module")
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mojo_simdjson_amd.device import Stage1Device

    d = Stage1Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def window(dev):
    """The tiny window's arrays from the real chain, the compiled path, and two zeroed inputs for what a refused call never
    reads (verdicts, records, a select result)"""
    import torch

    c = tvd.Chain(dev, WINDOW)
    paths = dev.compile_paths(["/a"])
    aux = [torch.zeros(32, dtype=torch.int64, device=dev.device) for _ in range(2)]
    args = dict(buf=c.d_buf.data_ptr(), len=c.length, idx=c.d_idx.data_ptr(), n=c.n, type=c.d_type.data_ptr(), depth=c.d_depth.data_ptr(),
                match=c.d_match.data_ptr(), end=c.d_end.data_ptr(), flags=c.d_flags.data_ptr(), first=c.d_first.data_ptr(),
                docs=c.d_docs.data_ptr(), numbers=c.d_numbers.data_ptr(), ncap=c.ncap, nres=c.d_num.data_ptr(), max_depth=100, cap=4,
                paths=paths.handle, aux0=aux[0].data_ptr(), aux1=aux[1].data_ptr())
    return c, paths, aux, args


@pytest.mark.parametrize("name", sorted(CALLS))
def test_two_faults(dev, window, name):
    import torch

    _, _, _, args = window
    order, output = CALLS[name]
    outs = {k: torch.full((32,), tvd.SENTINEL, dtype=torch.int64, device=dev.device) for k in ("out0", "out1", "out2", "out3", "res")}
    base = dict(args, **{k: t.data_ptr() for k, t in outs.items()})

    def call(**kw):
        a = dict(base, **kw)
        return getattr(dev.lib, name)(dev.ctx, *[a[k] for k in order], dev._stream())

    assert call(type=None, n=TOO_MANY) == BAD_ARGUMENT
    assert call(n=TOO_MANY, idx=base["idx"] + 4) == MSJ_CAPACITY
    assert call(**{output: None, "depth": base["depth"] + 4}) == BAD_ARGUMENT
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == tvd.SENTINEL).all()), k
