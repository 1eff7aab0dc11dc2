"""The library's error state across its translation units.  The gsr_* entry points are defined in many files of csrc/
(next to their kernels) and all report through gsr_entry.h's fail / hip_fail into ONE thread-local string, which
gsr_last_error() of gsr_api.hip returns.  Every call below is refused before any HIP call: no GPU is needed."""
import ctypes as C
import threading

BAD, CAPACITY = -1, -2


def _refusals(lib):
    """(call, code, exact message): one refusal in each of three files that hold their own entry points (mesh.hip,
    nearest.hip, model.hip) and one in gsr_api.hip."""
    buf = (C.c_char * 1024)()
    p = (C.addressof(buf) + 255) // 256 * 256
    R = 1000
    n_r, n_v = C.c_uint32(7), C.c_uint32(7)
    return buf, [
        (lambda: lib.gsr_mesh_cc_flatten(0, p, None), BAD, b"n must lie in 1..2^31-1"),
        (lambda: lib.gsr_nn_build(p, R, p, lib.gsr_nn_index_bytes(R) - 1, None), CAPACITY, b"nn index too small"),
        (lambda: lib.gsr_reset_opacity(p, 4, 1.5, None, None, None), BAD, b"cap must lie in (0, 1)"),
        (lambda: lib.gsr_forward_preprocess(None, None, None, None, C.byref(n_r), C.byref(n_v)), BAD, b"params is NULL"),
    ]


def test_every_file_reports_through_the_one_error_string_and_each_message_replaces_the_last():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    keep, refusals = _refusals(lib)
    messages = [m for _, _, m in refusals]
    assert len(set(messages)) == len(messages)
    # forwards, backwards and once more forwards: every file's message is seen right after every other file's
    for call, code, message in refusals + refusals[::-1] + refusals:
        assert call() == code
        assert lib.gsr_last_error() == message
        assert lib.gsr_last_error() == message, "reading the error must not clear it"
    del keep


def test_a_refusal_on_one_thread_leaves_a_fresh_thread_with_no_error():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    keep, refusals = _refusals(lib)
    seen = {}

    def fresh_thread():
        seen["before"] = lib.gsr_last_error()
        call, code, message = refusals[2]
        seen["rc"] = call()
        seen["after"] = lib.gsr_last_error()

    for call, code, message in (refusals[0], refusals[3]):          # one file that moved, and the one that stayed
        assert call() == code and lib.gsr_last_error() == message
        seen.clear()
        t = threading.Thread(target=fresh_thread)
        t.start()
        t.join()
        assert seen["before"] == b"", "a new thread starts with an empty error string"
        assert seen["rc"] == refusals[2][1] and seen["after"] == refusals[2][2]
        assert lib.gsr_last_error() == message, "the other thread's refusal must not show here"
    del keep
