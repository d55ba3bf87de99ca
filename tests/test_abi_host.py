"""The C ABI is stated once, in the headers (no GPU needed): the ctypes signatures `_native` reads from include/dronesim.h and
include/dronesim_verify.h are exactly the hand-written table they replaced (tests/golden/abi_signatures.json, recorded from that
table by tests/golden/gen_abi_signatures.py), so are the exported names and the constants; the parser refuses what it cannot read."""
import ctypes as C
import json
import os
import re

import pytest

from scalable_collision_avoidance_rl_amd import _native

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_signatures.json")))
LIBS = [("lib", _native.lib, "SYMBOLS", "SIGNATURES", "HEADER_PATH"),
        ("verify_lib", _native.verify_lib, "VERIFY_SYMBOLS", "VERIFY_SIGNATURES", "VERIFY_HEADER_PATH")]


def test_the_golden_holds_the_whole_abi():
    assert len(GOLDEN["lib"]) == 70 and len(GOLDEN["verify_lib"]) == 3


@pytest.mark.parametrize("key,load,symbols,signatures,header", LIBS, ids=[l[0] for l in LIBS])
def test_loaded_library_carries_exactly_the_recorded_signatures(key, load, symbols, signatures, header):
    lib, want = load(), GOLDEN[key]
    names = getattr(_native, symbols)
    assert isinstance(names, tuple) and len(set(names)) == len(names) and set(names) == set(want)
    text = open(getattr(_native, header)).read()
    for name in names:
        fn = getattr(lib, name)                                         # (AttributeError: the library does not export it)
        assert fn.restype.__name__ == want[name]["restype"], name
        assert [t.__name__ for t in fn.argtypes] == want[name]["argtypes"], name
        assert re.search(r"\b(int|const char \*)\s*%s\(" % name, text), name
    # header order: the names come out as the header declares them
    assert list(names) == sorted(names, key=lambda n: re.search(r"^(int |const char \*)%s\(" % n, text, re.M).start())


def test_pointer_kinds_are_the_classes_not_only_their_names():
    lib = _native.lib()
    assert lib.dronesim_step.argtypes[0] is C.POINTER(_native.DroneParams)
    assert lib.dronesim_step_ex.argtypes[1] is C.POINTER(_native.DroneEpisodeCtl)
    assert lib.dronesim_mlp_grad.argtypes[0] is C.POINTER(_native.DroneMlp)
    assert lib.dronesim_mlp_forward_bf16.argtypes[0] is C.POINTER(_native.DroneMlpBf16)
    assert lib.dronesim_mlp_grad_workspace.argtypes[2] is C.POINTER(C.c_size_t)
    assert _native.verify_lib().dronesim_step_f64.argtypes[0] is C.POINTER(_native.DroneParamsF64)
    # passed as plain integers on the step path: raw addresses, not mirrors
    assert list(lib.dronesim_step_call.argtypes) == [C.c_void_p] * 3 and lib.dronesim_episode_reduce.argtypes[0] is C.c_void_p
    assert lib.dronesim_last_error.restype is C.c_char_p and lib.dronesim_version.restype is C.c_int


def test_constants_are_the_recorded_values():
    assert {n: getattr(_native, n) for n in GOLDEN["constants"]} == GOLDEN["constants"]
    assert len(GOLDEN["constants"]) == 12


def test_exactly_the_entries_that_end_in_a_stream_are_marked():
    for key, _, symbols, signatures, _ in LIBS:
        sigs = getattr(_native, signatures)
        assert {n for n in sigs if not sigs[n].stream} == set(GOLDEN["no_stream"][key])
        assert all(sigs[n].argtypes[-1] is C.c_void_p for n in sigs if sigs[n].stream)
    # nine workspace queries, three block / stage counts, and the three that describe the library itself
    no = GOLDEN["no_stream"]["lib"]
    assert len(no) == 15 and sum(n.endswith("_workspace") for n in no) == 9


@pytest.mark.parametrize("text,what", [
    ("int dronesim_new_entry(const float *x, long n, void *stream);", "unknown parameter type 'long'"),        # a type it does not know
    ("float dronesim_new_entry(const float *x, void *stream);", "cannot read the declaration"),                # a return type it cannot read
    ("int dronesim_new_entry(int (*callback)(int), void *stream);", "cannot read the parameter"),              # a parameter it cannot read
])
def test_parser_raises_with_the_entry_name_and_never_guesses(text, what):
    with pytest.raises(ValueError, match="dronesim_new_entry: " + re.escape(what)):
        _native.parse_header("#define DRONESIM_OK 0\n" + text)


def test_parser_reads_comments_void_and_defines():
    constants, sigs = _native.parse_header("/* int dronesim_ghost(int a); */\n#define DRONESIM_A (-7)   /* c */\n#define DRONESIM_B 3\n"
                                           "// int dronesim_ghost2(void);\nconst char *dronesim_text(void);\n"
                                           "int dronesim_run(const DroneMlp *m, const void *const *src, size_t *n,\n    double e, void *stream);")
    assert constants == {"A": -7, "B": 3} and list(sigs) == ["dronesim_text", "dronesim_run"]
    assert sigs["dronesim_text"] == (C.c_char_p, [], False)
    assert sigs["dronesim_run"] == (C.c_int, [C.POINTER(_native.DroneMlp), C.c_void_p, C.POINTER(C.c_size_t), C.c_double, C.c_void_p], True)


def test_missing_header_is_an_import_error_naming_the_path(tmp_path):
    with pytest.raises(ImportError, match="no_such_header.h"):
        _native._read_header(str(tmp_path / "no_such_header.h"))


def test_workspace_queries_are_pure_host_calls():
    """No tensor, no device, no stream: a size query answers on a machine without a GPU."""
    assert _native.workspace("dronesim_standardize_workspace", 100, 4) > 0
    assert not _native.SIGNATURES["dronesim_standardize_workspace"].stream


def test_call_without_a_tensor_or_a_device_says_so():
    with pytest.raises(ValueError, match="dronesim_returns: no tensor argument and no device"):
        _native.call("dronesim_returns", None, None, 0.99, None, 0, 0, 1)
