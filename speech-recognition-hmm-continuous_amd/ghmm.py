"""ctypes binding of include/ghmm.h — the thin Python face of the C ABI.

Used by bench.py, __graft_entry__.py and tests/.  Nothing is computed here: every
call goes straight into libghmm_hip.so (HIP kernels) or, for the file-format /
synthetic-data helpers only, libghmm_host.so.  There is no CPU fallback for the
hot path: opening a context without the HIP library or without a gfx950 device
raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GHMM_HIP_LIB: a measurement build of the library (profiles/tools/lab.sh); default = the product
HIP_LIB = os.environ.get("GHMM_HIP_LIB") or os.path.join(_HERE, "libghmm_hip.so")
HOST_LIB = os.path.join(_HERE, "libghmm_host.so")

OK = 0
ERR_ARG, ERR_ALLOC, ERR_HIP, ERR_NODEVICE, ERR_UNSUPPORTED, ERR_IO, ERR_FORMAT = range(1, 8)
(OPT_DELTA, OPT_ROBUST, OPT_KERNELS, OPT_TIMING, OPT_PARTIALS, OPT_CUS, OPT_REFORDER_COUNT, OPT_VEC_STATS,
 OPT_NT_POST, OPT_FUSED_SCAN) = range(1, 11)
(K_EMISSION, K_FORWARD, K_BACKWARD, K_MIXSTATS, K_REDUCE, K_MSTEP, K_VITERBI, K_PREPARE,
 K_COUNT) = range(9)
(BUF_B, BUF_POST, BUF_ALPHA, BUF_BETA, BUF_SCALE, BUF_GAMMA, BUF_LOGLIK, BUF_LOGNORM) = range(8)
SYNTH_SEED = 20260104
MAX_WORD = 256

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p


class GhmmError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        super().__init__(f"ghmm error {code}: {detail}")


class HostModelStruct(C.Structure):
    _fields_ = [("word", C.c_char * MAX_WORD), ("N", C.c_int), ("M", C.c_int), ("D", C.c_int),
                ("A", _dp), ("c", _dp), ("mean", _dp), ("inv_var", _dp), ("det", _dp)]


class HostFullModelStruct(C.Structure):
    _fields_ = [("word", C.c_char * MAX_WORD), ("N", C.c_int), ("M", C.c_int), ("D", C.c_int),
                ("A", _dp), ("c", _dp), ("mean", _dp), ("det", _dp), ("inv_cov", _dp)]


# every exported symbol of include/ghmm.h: name -> (restype, argtypes, needs_hip)
SYMBOLS = {
    "ghmm_strerror": (C.c_char_p, [C.c_int], False),
    "ghmm_last_error": (C.c_char_p, [], False),
    "ghmm_version": (C.c_int, [], False),
    "ghmm_ctx_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)], True),
    "ghmm_ctx_destroy": (None, [_vp], True),
    "ghmm_ctx_sync": (C.c_int, [_vp], True),
    "ghmm_ctx_set_option": (C.c_int, [_vp, C.c_int, C.c_int64], True),
    "ghmm_ctx_get_option": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64)], True),
    "ghmm_ctx_kernel_time": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(C.c_int64)], True),
    "ghmm_ctx_kernel_time_reset": (C.c_int, [_vp], True),
    "ghmm_kernel_name": (C.c_char_p, [C.c_int], True),
    "ghmm_model_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)], True),
    "ghmm_model_destroy": (None, [_vp, _vp], True),
    "ghmm_model_set": (C.c_int, [_vp, _vp, _dp, _dp, _dp, _dp, _dp], True),
    "ghmm_model_get": (C.c_int, [_vp, _vp, _dp, _dp, _dp, _dp, _dp], True),
    "ghmm_model_init": (C.c_int, [_vp, _vp, _vp], True),
    "ghmm_model_init_comm": (C.c_int, [_vp, _vp, _vp, _vp], True),
    "ghmm_comm_unique_id": (C.c_int, [_vp], True),
    "ghmm_comm_create": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)], True),
    "ghmm_comm_create_file": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_double,
                                        C.POINTER(_vp)], True),
    "ghmm_comm_destroy": (None, [_vp], True),
    "ghmm_comm_rank": (C.c_int, [_vp], True),
    "ghmm_comm_size": (C.c_int, [_vp], True),
    "ghmm_stats_allreduce": (C.c_int, [_vp, _vp, _vp], True),
    "ghmm_model_dims": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int)], True),
    "ghmm_corpus_create": (C.c_int, [_vp, _dp, _ip, C.c_int, C.c_int, C.POINTER(_vp)], True),
    "ghmm_corpus_wrap": (C.c_int, [_vp, _vp, _ip, C.c_int, C.c_int, C.POINTER(_vp)], True),
    "ghmm_corpus_destroy": (None, [_vp, _vp], True),
    "ghmm_corpus_frames": (C.c_int64, [_vp], True),
    "ghmm_corpus_utterances": (C.c_int, [_vp], True),
    "ghmm_stats_len": (C.c_size_t, [C.c_int, C.c_int, C.c_int], True),
    "ghmm_stats_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)], True),
    "ghmm_stats_wrap": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(_vp)], True),
    "ghmm_stats_destroy": (None, [_vp, _vp], True),
    "ghmm_stats_device_ptr": (_vp, [_vp], True),
    "ghmm_stats_download": (C.c_int, [_vp, _vp, _dp], True),
    "ghmm_stats_upload": (C.c_int, [_vp, _vp, _dp], True),
    "ghmm_stats_loglik": (C.c_int, [_vp, _vp, _dp], True),
    "ghmm_emission": (C.c_int, [_vp, _vp, _vp, C.c_int], True),
    "ghmm_forward": (C.c_int, [_vp, _vp, _vp], True),
    "ghmm_backward": (C.c_int, [_vp, _vp, _vp], True),
    "ghmm_accumulate": (C.c_int, [_vp, _vp, _vp, _vp], True),
    "ghmm_fetch": (C.c_int, [_vp, C.c_int, _dp, C.c_size_t], True),
    "ghmm_fetch_range": (C.c_int, [_vp, C.c_int, C.c_size_t, _dp, C.c_size_t], True),
    "ghmm_estep": (C.c_int, [_vp, _vp, _vp, _vp], True),
    "ghmm_mstep": (C.c_int, [_vp, _vp, _vp], True),
    "ghmm_mstep_ebw": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double], True),
    "ghmm_score": (C.c_int, [_vp, _vp, _vp, _dp], True),
    "ghmm_score_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, _vp, _dp], True),
    "ghmm_estep_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, C.POINTER(_vp)], True),
    "ghmm_score_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, _dp], True),
    "ghmm_viterbi": (C.c_int, [_vp, _vp, _vp, _ip, _dp], True),
    "ghmm_viterbi_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, _ip, _dp], True),
    "ghmm_score_streams_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp], True),
    "ghmm_viterbi_streams_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp], True),
    "ghmm_recognise_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _ip, _ip, _dp],
                               True),
    "ghmm_connect_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, C.c_double, _ip, _ip,
                                       _ip, _dp], True),
    "ghmm_connect_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, C.c_double, _ip,
                                            _ip, _ip, _dp], True),
    "ghmm_connect_grammar_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp, _dp, _dp,
                                               _ip, _ip, _ip, _dp], True),
    "ghmm_connect_grammar_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp, _dp,
                                                    _dp, _ip, _ip, _ip, _dp], True),
    "ghmm_grammar_post_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp, _dp, _dp,
                                            _dp, _dp, _dp], True),
    "ghmm_grammar_post_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp, _dp,
                                                 _dp, _dp, _dp, _dp], True),
    "ghmm_align_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _ip, _ip, _ip, _ip, _ip,
                                     _dp], True),
    "ghmm_estep_embed_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _ip, _ip,
                                           C.POINTER(_vp)], True),
    "ghmm_estep_grammar_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp, _dp, _dp,
                                             C.POINTER(_vp)], True),
    "ghmm_align_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _ip, _ip, _ip, _ip,
                                          _ip, _dp], True),
    "ghmm_estep_embed_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _ip, _ip,
                                                C.POINTER(_vp)], True),
    "ghmm_logscore": (C.c_int, [_vp, _vp, _vp, C.c_int, _dp], True),
    "ghmm_logscore_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, _vp, C.c_int, _dp], True),
    "ghmm_logscore_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, C.c_int, _dp], True),
    "ghmm_estep_log": (C.c_int, [_vp, _vp, _vp, _vp], True),
    "ghmm_estep_log_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, C.POINTER(_vp)], True),
    "ghmm_logscore_streams_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, C.c_int, _dp],
                                    True),
    "ghmm_fmodel_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)], True),
    "ghmm_fmodel_destroy": (None, [_vp, _vp], True),
    "ghmm_fmodel_set": (C.c_int, [_vp, _vp, _dp, _dp, _dp, _dp, _dp], True),
    "ghmm_fmodel_get": (C.c_int, [_vp, _vp, _dp, _dp, _dp, _dp, _dp], True),
    "ghmm_fmodel_dims": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)], True),
    "ghmm_emission_full": (C.c_int, [_vp, _vp, _vp], True),
    "ghmm_score_full": (C.c_int, [_vp, _vp, _vp, _dp], True),
    "ghmm_score_full_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, _vp, _dp], True),
    "ghmm_viterbi_full": (C.c_int, [_vp, _vp, _vp, _ip, _dp], True),
    "ghmm_viterbi_full_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, _vp, _dp], True),
    "ghmm_logscore_full": (C.c_int, [_vp, _vp, _vp, C.c_int, _dp], True),
    "ghmm_logscore_full_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, _vp, C.c_int, _dp], True),
    "ghmm_stats_len_full": (C.c_size_t, [C.c_int, C.c_int, C.c_int], False),
    "ghmm_stats_create_full": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)], True),
    "ghmm_estep_full": (C.c_int, [_vp, _vp, _vp, _vp], True),
    "ghmm_estep_full_log": (C.c_int, [_vp, _vp, _vp, _vp], True),
    "ghmm_mstep_full": (C.c_int, [_vp, _vp, _vp], True),
    "ghmm_mstep_full_dev": (C.c_int, [_vp, _vp, _vp], True),
    "ghmm_fmodel_init": (C.c_int, [_vp, _vp, _vp, _vp], True),
    "ghmm_estep_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, C.POINTER(_vp),
                                          C.c_int], True),
    "ghmm_score_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, _dp], True),
    "ghmm_logscore_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, C.c_int, _dp],
                                   True),
    "ghmm_viterbi_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.c_int, _ip, _dp], True),
    "ghmm_score_full_streams_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp],
                                      True),
    "ghmm_logscore_full_streams_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int,
                                                   C.c_int, _dp], True),
    "ghmm_viterbi_full_streams_batch": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _dp],
                                        True),
    "ghmm_recognise_full_streams": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, _ip, _ip,
                                              _dp], True),
    "ghmm_perfil_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(_dp)], False),
    "ghmm_perfil_write": (C.c_int, [C.c_char_p, C.c_int, C.c_int, _dp], False),
    "ghmm_perfil_stat": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)], False),
    "ghmm_shard_balanced": (C.c_int, [_ip, C.c_int, C.c_int, C.c_int, _ip, C.POINTER(C.c_int)],
                            False),
    "ghmm_rendezvous_file": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_double, _vp], False),
    "ghmm_free": (None, [_vp], False),
    "ghmm_host_model_alloc": (C.c_int, [C.POINTER(HostModelStruct), C.c_int, C.c_int, C.c_int],
                              False),
    "ghmm_host_model_free": (None, [C.POINTER(HostModelStruct)], False),
    "ghmm_hmm_read": (C.c_int, [C.c_char_p, C.POINTER(HostModelStruct)], False),
    "ghmm_hmm_write": (C.c_int, [C.c_char_p, C.POINTER(HostModelStruct), C.c_int], False),
    "ghmm_hmm_read_streams": (C.c_int, [C.c_char_p, C.POINTER(HostModelStruct), C.c_int,
                                        C.POINTER(C.c_int)], False),
    "ghmm_hmm_write_streams": (C.c_int, [C.c_char_p, C.POINTER(HostModelStruct), C.c_int, C.c_int],
                               False),
    "ghmm_host_fmodel_alloc": (C.c_int, [C.POINTER(HostFullModelStruct), C.c_int, C.c_int, C.c_int],
                               False),
    "ghmm_host_fmodel_free": (None, [C.POINTER(HostFullModelStruct)], False),
    "ghmm_hmm_read_full": (C.c_int, [C.c_char_p, C.POINTER(HostFullModelStruct)], False),
    "ghmm_hmm_write_full": (C.c_int, [C.c_char_p, C.POINTER(HostFullModelStruct), C.c_int], False),
    "ghmm_hmm_read_full_streams": (C.c_int, [C.c_char_p, C.POINTER(HostFullModelStruct), C.c_int,
                                             C.POINTER(C.c_int)], False),
    "ghmm_hmm_write_full_streams": (C.c_int, [C.c_char_p, C.POINTER(HostFullModelStruct), C.c_int,
                                              C.c_int], False),
    "ghmm_init_model": (C.c_int, [_dp, _ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(HostModelStruct)], False),
    "ghmm_init_model_full": (C.c_int, [_dp, _ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(HostFullModelStruct)], False),
    "ghmm_mstep_full_host": (C.c_int, [_dp, C.c_int, C.POINTER(HostFullModelStruct)], False),
    "ghmm_inv_cov_full": (C.c_double, [C.c_int, _dp], False),
    "ghmm_synth_truth": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, _dp, _dp], False),
    "ghmm_synth_utterances": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                        C.c_int64, C.c_int, _ip, _dp], False),
    "ghmm_synth_start_model": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                         C.c_double, _dp, _dp, _dp, _dp, _dp], False),
}

_libs = {}


def _bind(lib, hip):
    for name, (res, args, needs_hip) in SYMBOLS.items():
        if needs_hip and not hip:
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def hip_lib():
    """The C-ABI library with the HIP kernels.  Raises if it has not been built."""
    if "hip" not in _libs:
        if not os.path.exists(HIP_LIB):
            raise GhmmError(ERR_NODEVICE, f"{HIP_LIB} is missing — run __graft_entry__.build(); "
                                          "the hot path has no CPU fallback")
        _libs["hip"] = _bind(C.CDLL(HIP_LIB), True)
    return _libs["hip"]


def host_lib():
    """Host-only helpers (file formats, init model, synthetic corpora)."""
    if "host" not in _libs:
        if os.path.exists(HIP_LIB):
            _libs["host"] = hip_lib()
        else:
            _libs["host"] = _bind(C.CDLL(HOST_LIB), False)
    return _libs["host"]


def _check(rc, lib):
    if rc != OK:
        raise GhmmError(rc, (lib.ghmm_last_error() or b"").decode() or
                        lib.ghmm_strerror(rc).decode())


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


class HostModel:
    """A model in host memory: the flat struct-of-arrays of include/ghmm.h."""

    def __init__(self, A, c, mean, inv_var, det, word=""):
        self.A = _f64(A)
        self.N = self.A.shape[0]
        self.c = _f64(c).reshape(self.N, -1)
        self.M = self.c.shape[1]
        self.mean = _f64(mean).reshape(self.N, self.M, -1)
        self.D = self.mean.shape[2]
        self.inv_var = _f64(inv_var).reshape(self.N, self.M, self.D)
        self.det = _f64(det).reshape(self.N, self.M)
        self.word = word

    def copy(self):
        return HostModel(self.A.copy(), self.c.copy(), self.mean.copy(), self.inv_var.copy(),
                         self.det.copy(), self.word)

    def arrays(self):
        return self.A, self.c, self.mean, self.inv_var, self.det

    def _struct(self):
        s = HostModelStruct()
        s.word = self.word.encode()[:MAX_WORD - 1]
        s.N, s.M, s.D = self.N, self.M, self.D
        s.A, s.c, s.mean, s.inv_var, s.det = (_d(x) for x in self.arrays())
        return s

    @staticmethod
    def _from_struct(s, lib):
        N, M, D = s.N, s.M, s.D
        G = N * M
        hm = HostModel(np.ctypeslib.as_array(s.A, (N, N)).copy(),
                       np.ctypeslib.as_array(s.c, (N, M)).copy(),
                       np.ctypeslib.as_array(s.mean, (N, M, D)).copy(),
                       np.ctypeslib.as_array(s.inv_var, (N, M, D)).copy(),
                       np.ctypeslib.as_array(s.det, (G,)).copy(), s.word.decode())
        lib.ghmm_host_model_free(C.byref(s))
        return hm

    @staticmethod
    def read(path):
        lib = host_lib()
        s = HostModelStruct()
        _check(lib.ghmm_hmm_read(os.fsencode(path), C.byref(s)), lib)
        return HostModel._from_struct(s, lib)

    def write(self, path, len_bytes=8):
        lib = host_lib()
        s = self._struct()
        _check(lib.ghmm_hmm_write(os.fsencode(path), C.byref(s), len_bytes), lib)

    @staticmethod
    def read_streams(path, max_streams=8):
        """A model of several feature streams (param_number P): one HostModel per stream."""
        lib = host_lib()
        arr = (HostModelStruct * max_streams)()
        n = C.c_int()
        _check(lib.ghmm_hmm_read_streams(os.fsencode(path), arr, max_streams, C.byref(n)), lib)
        return [HostModel._from_struct(arr[p], lib) for p in range(n.value)]

    @staticmethod
    def write_streams(path, hms, len_bytes=8):
        lib = host_lib()
        arr = (HostModelStruct * len(hms))(*[h._struct() for h in hms])
        _check(lib.ghmm_hmm_write_streams(os.fsencode(path), arr, len(hms), len_bytes), lib)

    @staticmethod
    def init_from(X, lens, N, M):
        """creating_initial_model (TF:732) on in-memory utterances."""
        lib = host_lib()
        X = _f64(X)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        s = HostModelStruct()
        _check(lib.ghmm_init_model(_d(X), lens.ctypes.data_as(_ip), len(lens), N, M, X.shape[1],
                                   C.byref(s)), lib)
        return HostModel._from_struct(s, lib)


class HostFullModel:
    """A full-covariance model in host memory (ghmm_host_fmodel): inv_cov[N, M, D, D] where
    HostModel has inv_var[N, M, D]; det is that of the non-inverted covariance."""

    def __init__(self, A, c, mean, inv_cov, det, word=""):
        self.A = _f64(A)
        self.N = self.A.shape[0]
        self.c = _f64(c).reshape(self.N, -1)
        self.M = self.c.shape[1]
        self.mean = _f64(mean).reshape(self.N, self.M, -1)
        self.D = self.mean.shape[2]
        self.inv_cov = _f64(inv_cov).reshape(self.N, self.M, self.D, self.D)
        self.det = _f64(det).reshape(self.N, self.M)
        self.word = word

    def arrays(self):
        """(A, c, mean, inv_cov, det): the argument order of ghmm_fmodel_set"""
        return self.A, self.c, self.mean, self.inv_cov, self.det

    def copy(self):
        return HostFullModel(self.A.copy(), self.c.copy(), self.mean.copy(), self.inv_cov.copy(),
                             self.det.copy(), self.word)

    @staticmethod
    def _from_struct(s, lib):
        N, M, D = s.N, s.M, s.D
        hm = HostFullModel(np.ctypeslib.as_array(s.A, (N, N)).copy(),
                           np.ctypeslib.as_array(s.c, (N, M)).copy(),
                           np.ctypeslib.as_array(s.mean, (N, M, D)).copy(),
                           np.ctypeslib.as_array(s.inv_cov, (N, M, D, D)).copy(),
                           np.ctypeslib.as_array(s.det, (N, M)).copy(), s.word.decode())
        lib.ghmm_host_fmodel_free(C.byref(s))
        return hm

    @staticmethod
    def init_from(X, lens, N, M):
        """creating_initial_model of the full-covariance trainer (TFF:731) on in-memory utterances
        (ghmm_init_model_full)."""
        lib = host_lib()
        X = _f64(X)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        s = HostFullModelStruct()
        _check(lib.ghmm_init_model_full(_d(X), lens.ctypes.data_as(_ip), len(lens), N, M, X.shape[1],
                                        C.byref(s)), lib)
        return HostFullModel._from_struct(s, lib)

    def mstep(self, stats, delta=1):
        """ghmm_mstep_full_host: the M-step of TFF (TFF:306-341) from a full statistics vector;
        returns the new model (this one is left as it is)."""
        lib = host_lib()
        out = self.copy()
        v = _f64(stats)
        assert v.size == stats_len_full(self.N, self.M, self.D)
        _check(lib.ghmm_mstep_full_host(_d(v), int(delta), C.byref(out._struct())), lib)
        return out

    def _struct(self):
        s = HostFullModelStruct()
        s.word = self.word.encode()[:MAX_WORD - 1]
        s.N, s.M, s.D = self.N, self.M, self.D
        s.A, s.c, s.mean, s.det, s.inv_cov = (_d(x) for x in (self.A, self.c, self.mean, self.det,
                                                               self.inv_cov))
        return s

    @staticmethod
    def read(path):
        lib = host_lib()
        s = HostFullModelStruct()
        _check(lib.ghmm_hmm_read_full(os.fsencode(path), C.byref(s)), lib)
        return HostFullModel._from_struct(s, lib)

    def write(self, path, len_bytes=8):
        lib = host_lib()
        s = self._struct()
        _check(lib.ghmm_hmm_write_full(os.fsencode(path), C.byref(s), len_bytes), lib)

    @staticmethod
    def read_streams(path, max_streams=8):
        """A full-covariance model of several feature streams (param_number P): one HostFullModel per
        stream, each with the common word, N and A (ghmm_hmm_read_full_streams)."""
        lib = host_lib()
        arr = (HostFullModelStruct * max_streams)()
        n = C.c_int()
        _check(lib.ghmm_hmm_read_full_streams(os.fsencode(path), arr, max_streams, C.byref(n)), lib)
        return [HostFullModel._from_struct(arr[p], lib) for p in range(n.value)]

    @staticmethod
    def write_streams(path, hfms, len_bytes=8):
        """word, N and A are written from hfms[0] (ghmm_hmm_write_full_streams)"""
        lib = host_lib()
        arr = (HostFullModelStruct * len(hfms))(*[h._struct() for h in hfms])
        _check(lib.ghmm_hmm_write_full_streams(os.fsencode(path), arr, len(hfms), len_bytes), lib)


def inv_cov_full(cov):
    """ghmm_inv_cov_full (TFF's inv_cov_matrix): (det, matrix) — the inverse, or the matrix as it
    came where det == 0"""
    a = _f64(cov).copy()
    det = host_lib().ghmm_inv_cov_full(a.shape[0], _d(a))
    return det, a


def perfil_read(path):
    lib = host_lib()
    D, T, p = C.c_int(), C.c_int(), _dp()
    _check(lib.ghmm_perfil_read(os.fsencode(path), C.byref(D), C.byref(T), C.byref(p)), lib)
    X = np.ctypeslib.as_array(p, (T.value, D.value)).copy() if T.value else np.zeros((0, D.value))
    lib.ghmm_free(p)
    return X


def perfil_stat(path):
    """(D, T) of a .perfil file from its header and size."""
    lib = host_lib()
    D, T = C.c_int(), C.c_int()
    _check(lib.ghmm_perfil_stat(os.fsencode(path), C.byref(D), C.byref(T)), lib)
    return D.value, T.value


def shard_balanced(lens, rank, world):
    """ghmm_shard_balanced: this rank's utterance indices (ascending), length-balanced."""
    lib = host_lib()
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    idx = np.empty((len(lens) + world - 1) // world + 1, dtype=np.int32)
    n = C.c_int()
    _check(lib.ghmm_shard_balanced(lens.ctypes.data_as(_ip), len(lens), rank, world,
                                   idx.ctypes.data_as(_ip), C.byref(n)), lib)
    return idx[:n.value].copy()


def perfil_write(path, X):
    lib = host_lib()
    X = _f64(X)
    _check(lib.ghmm_perfil_write(os.fsencode(path), X.shape[1], X.shape[0], _d(X)), lib)


def synth_truth(N, M, D, seed=SYNTH_SEED):
    lib = host_lib()
    mean = np.empty((N, M, D))
    std = np.empty((N, M, D))
    _check(lib.ghmm_synth_truth(seed, N, M, D, _d(mean), _d(std)), lib)
    return mean, std


def synth_utterances(mean, std, lens, first_utt=0, seed=SYNTH_SEED, threads=1):
    """Utterance u depends only on (seed, first_utt + u) (ghmm_synth.c), so `threads` > 1 deals
    contiguous blocks of utterances to host threads (the C call releases the GIL): same bytes."""
    lib = host_lib()
    N, M, D = mean.shape
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    X = np.empty((int(lens.sum()), D))
    U = len(lens)
    threads = max(1, min(int(threads), U))

    def block(lo, hi, f0):
        ln = np.ascontiguousarray(lens[lo:hi])
        _check(lib.ghmm_synth_utterances(seed, N, M, D, _d(mean), _d(std), first_utt + lo, hi - lo,
                                         ln.ctypes.data_as(_ip), _d(X[f0:])), lib)

    if threads == 1:
        block(0, U, 0)
        return X
    import threading
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    cuts = [U * k // threads for k in range(threads + 1)]
    errs = []

    def run(lo, hi):
        try:
            block(lo, hi, int(off[lo]))
        except BaseException as e:   # noqa: BLE001 - re-raised below on the caller's thread
            errs.append(e)

    ts = [threading.Thread(target=run, args=(cuts[k], cuts[k + 1])) for k in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    return X


def synth_start_model(mean, std, perturb=0.05, seed=SYNTH_SEED):
    lib = host_lib()
    N, M, D = mean.shape
    A = np.empty((N, N)); c = np.empty((N, M)); mu = np.empty((N, M, D))
    iv = np.empty((N, M, D)); det = np.empty((N, M))
    _check(lib.ghmm_synth_start_model(seed, N, M, D, _d(mean), _d(std), perturb, _d(A), _d(c),
                                      _d(mu), _d(iv), _d(det)), lib)
    return HostModel(A, c, mu, iv, det, "synth")


def rendezvous_file(path, rank, world, timeout_s=120.0, id_bytes=None):
    """ghmm_rendezvous_file: rank 0 passes the 128-byte id, the other ranks get it back."""
    lib = host_lib()
    buf = C.create_string_buffer(id_bytes if id_bytes is not None else b"", 128)
    _check(lib.ghmm_rendezvous_file(os.fsencode(path), rank, world, float(timeout_s), buf), lib)
    return buf.raw


def word_segments(word, begin, lens):
    """What connect_streams decoded, per utterance the list of (word, first_frame, last_frame) with the
    frames counted inside the utterance: a word instance runs from a frame with begin == 1 to the frame
    before the next one.  An empty utterance gives an empty list."""
    out, f0 = [], 0
    for T in lens:
        T = int(T)
        starts = [t for t in range(T) if begin[f0 + t]]
        if T and (not starts or starts[0] != 0):
            raise ValueError("an utterance's first frame must begin a word")
        ends = [t - 1 for t in starts[1:]] + [T - 1]
        out.append([(int(word[f0 + a]), a, b) for a, b in zip(starts, ends)])
        f0 += T
    return out


def word_confidence(segments, occ, lens):
    """A confidence per decoded word: segments = word_segments(word, begin, lens) of a connected-word decoding,
    occ[F, K] = grammar_post_streams' frame posteriors of the same corpus and grammar.  Per utterance the list
    of (word, first, last, confidence), confidence = the mean of occ[f0 + first .. f0 + last, word] with f0 the
    utterance's first frame: the average posterior that the instance's frames lie in its word."""
    occ = np.asarray(occ)
    if len(segments) != len(lens):
        raise ValueError(f"{len(segments)} segment lists for {len(lens)} utterances")
    out, f0 = [], 0
    for segs, T in zip(segments, lens):
        T = int(T)
        row = []
        for k, a, b in segs:
            if not 0 <= a <= b < T:
                raise ValueError(f"segment ({k}, {a}, {b}) outside an utterance of {T} frames")
            row.append((int(k), int(a), int(b), float(occ[f0 + a:f0 + b + 1, k].mean())))
        out.append(row)
        f0 += T
    return out


def bigram_log(transcripts, n_words, alpha=1.0):
    """A word-pair grammar for connect_grammar_streams estimated from transcripts (sequences of word
    indices below n_words; empty ones are skipped): (start[K], pair[K, K], fin[K]) in natural logs, K =
    n_words.  Counts: s[k] = the transcripts that open with k; c[w, k] = the times k follows w; f[w] =
    the transcripts that close with w (the end of a transcript is one more event of its last word's
    row).  With additive smoothing alpha >= 0:
        start[k]   = log((s[k]    + alpha) / (sum_k' s[k']            + alpha * K))
        pair[w, k] = log((c[w, k] + alpha) / (sum_k' c[w, k'] + f[w]  + alpha * (K + 1)))
        fin[w]     = log((f[w]    + alpha) / (sum_k' c[w, k'] + f[w]  + alpha * (K + 1)))
    so that exp(start) sums to 1 and every row of exp(pair) together with exp(fin) of that row sums to 1.
    A zero numerator gives -inf (alpha = 0: unseen events are forbidden), a row without any event as well."""
    K = int(n_words)
    if K < 1 or alpha < 0:
        raise ValueError("bigram_log: n_words >= 1 and alpha >= 0")
    s, c, f = np.zeros(K), np.zeros((K, K)), np.zeros(K)
    for t in transcripts:
        t = [int(k) for k in t]
        if any(not 0 <= k < K for k in t):
            raise ValueError(f"bigram_log: a word outside 0 .. {K - 1} in {t}")
        if not t:
            continue
        s[t[0]] += 1
        for w, k in zip(t[:-1], t[1:]):
            c[w, k] += 1
        f[t[-1]] += 1

    def log_ratio(num, den):
        num, den = np.broadcast_arrays(np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64))
        out = np.full(num.shape, -np.inf)
        ok = (num > 0) & (den > 0)
        out[ok] = np.log(num[ok] / den[ok])
        return out

    row = c.sum(1) + f + alpha * (K + 1)
    return log_ratio(s + alpha, s.sum() + alpha * K), log_ratio(c + alpha, row[:, None]), log_ratio(f + alpha, row)


def cut_segments(Xs, lens, segments, n_words, score=None):
    """A connected corpus cut at word_segments' boundaries into one isolated-word corpus per word, what
    Corpus and the trainers accept: Xs[p] = stream p's frames [F][D_p], lens[u] = utterance u's frames,
    segments = word_segments(word, begin, lens).  Returns per word k = 0 .. n_words-1 the pair
    (Xs_k, lens_k): Xs_k[p] = the frames of k's instances one after the other in stream p (utterance by
    utterance, in time order), lens_k the instances' lengths; a word that never occurs has arrays of no
    frames.  With score given (align_streams' per utterance) an utterance whose score is not finite is
    left out: its alignment carries no meaning."""
    Xs = [np.asarray(X) for X in Xs]
    parts = [[[] for _ in Xs] for _ in range(n_words)]
    out_lens = [[] for _ in range(n_words)]
    f0 = 0
    for u, T in enumerate(lens):
        T = int(T)
        if score is None or np.isfinite(score[u]):
            for k, a, b in segments[u]:
                if not (0 <= k < n_words and 0 <= a <= b < T):
                    raise ValueError(f"utterance {u}: segment {(k, a, b)} outside {n_words} words or {T} frames")
                for p, X in enumerate(Xs):
                    parts[k][p].append(X[f0 + a:f0 + b + 1])
                out_lens[k].append(b - a + 1)
        f0 += T
    return [([np.concatenate(parts[k][p]) if parts[k][p] else X[:0].copy() for p, X in enumerate(Xs)],
             np.asarray(out_lens[k], dtype=np.int32)) for k in range(n_words)]


def stats_len(N, M, D):
    return N * N + 2 * N + N * M * (2 * D + 1) + 2


def split_stats(v, N, M, D):
    """Views into a flat statistics vector (layout of include/ghmm.h)."""
    G = N * M
    o = 0
    out = {}
    for name, n, shape in (("num_a", N * N, (N, N)), ("den_a", N, (N,)), ("den_c", N, (N,)),
                           ("num_c", G, (N, M)), ("num_mu", G * D, (N, M, D)),
                           ("num_var", G * D, (N, M, D)), ("loglik", 1, ()), ("n_utt", 1, ())):
        out[name] = v[o:o + n].reshape(shape)
        o += n
    return out


def stats_len_full(N, M, D):
    return N * N + 2 * N + N * M * (1 + D + D * (D + 1) // 2) + 2


def split_stats_full(v, N, M, D):
    """Views into a full-covariance statistics vector (ghmm_stats_create_full); num_cov holds the
    upper triangle (k <= l, row-major) of every Gaussian, in numpy.triu_indices(D) order."""
    G, DT = N * M, D * (D + 1) // 2
    o = 0
    out = {}
    for name, n, shape in (("num_a", N * N, (N, N)), ("den_a", N, (N,)), ("den_c", N, (N,)),
                           ("num_c", G, (N, M)), ("num_mu", G * D, (N, M, D)),
                           ("num_cov", G * DT, (N, M, DT)), ("loglik", 1, ()), ("n_utt", 1, ())):
        out[name] = v[o:o + n].reshape(shape)
        o += n
    return out


class Context:
    """One GPU, one stream.  `stream` = a hipStream_t as int (e.g. torch's
    torch.cuda.current_stream().cuda_stream) or None for a private stream."""

    def __init__(self, device=0, stream=None):
        self.lib = hip_lib()
        h = _vp()
        _check(self.lib.ghmm_ctx_create(device, _vp(stream) if stream else None, C.byref(h)),
               self.lib)
        self.h = h
        self._children = []

    def close(self):
        if self.h:
            for ch in self._children:
                ch.close()
            self.lib.ghmm_ctx_destroy(self.h)
            self.h = None

    def sync(self):
        _check(self.lib.ghmm_ctx_sync(self.h), self.lib)

    def set_option(self, opt, value):
        _check(self.lib.ghmm_ctx_set_option(self.h, opt, int(value)), self.lib)

    def get_option(self, opt):
        v = C.c_int64()
        _check(self.lib.ghmm_ctx_get_option(self.h, opt, C.byref(v)), self.lib)
        return v.value

    def kernel_times(self):
        out = {}
        for k in range(K_COUNT):
            ms, n = C.c_double(), C.c_int64()
            _check(self.lib.ghmm_ctx_kernel_time(self.h, k, C.byref(ms), C.byref(n)), self.lib)
            out[self.lib.ghmm_kernel_name(k).decode()] = (ms.value, n.value)
        return out

    def kernel_times_reset(self):
        _check(self.lib.ghmm_ctx_kernel_time_reset(self.h), self.lib)

    # ---- objects
    def model(self, hm):
        return Model(self, hm)

    def corpus(self, X, lens):
        return Corpus(self, X, lens)

    def corpus_from_device(self, dev_ptr, lens, D):
        return Corpus(self, None, lens, dev_ptr=dev_ptr, D=D)

    def stats(self, N, M, D, dev_ptr=None):
        return Stats(self, N, M, D, dev_ptr)

    def stats_full(self, N, M, D):
        """statistics vector of the full-covariance trainer (ghmm_stats_create_full)"""
        return Stats(self, N, M, D, full=True)

    # ---- the path, row by row
    def emission(self, model, corpus, want_post=True):
        _check(self.lib.ghmm_emission(self.h, model.h, corpus.h, int(want_post)), self.lib)

    def forward(self, model, corpus):
        _check(self.lib.ghmm_forward(self.h, model.h, corpus.h), self.lib)

    def backward(self, model, corpus):
        _check(self.lib.ghmm_backward(self.h, model.h, corpus.h), self.lib)

    def accumulate(self, model, corpus, stats):
        _check(self.lib.ghmm_accumulate(self.h, model.h, corpus.h, stats.h), self.lib)

    def fetch(self, which, shape):
        out = np.empty(shape, dtype=np.float64)
        _check(self.lib.ghmm_fetch(self.h, which, _d(out), out.size), self.lib)
        return out

    def fetch_range(self, which, first, shape):
        """doubles [first, first + prod(shape)) of a workspace buffer"""
        out = np.empty(shape, dtype=np.float64)
        _check(self.lib.ghmm_fetch_range(self.h, which, int(first), _d(out), out.size), self.lib)
        return out

    # ---- several GPUs
    def comm(self, rank=0, world=1, id_bytes=None, path=None, timeout_s=120.0):
        return Comm(self, rank, world, id_bytes, path, timeout_s)

    def stats_allreduce(self, stats, comm):
        _check(self.lib.ghmm_stats_allreduce(self.h, stats.h, comm.h), self.lib)

    # ---- fused
    def estep(self, model, corpus, stats):
        _check(self.lib.ghmm_estep(self.h, model.h, corpus.h, stats.h), self.lib)

    def estep_log(self, model, corpus, stats):
        """the same E-step in the log domain (ghmm_estep_log): finite where estep's linear densities
        underflow on a whole frame"""
        _check(self.lib.ghmm_estep_log(self.h, model.h, corpus.h, stats.h), self.lib)

    def mstep(self, model, stats):
        _check(self.lib.ghmm_mstep(self.h, model.h, stats.h), self.lib)

    def mstep_ebw(self, model, num, den, E=2.0):
        """the extended Baum-Welch update in place: means and variances from the numerator vector `num`
        (the transcripts' statistics) against the denominator vector `den` (estep_grammar_streams'), damped per
        Gaussian by max(E * den.num_c, twice the value that keeps every variance positive); weights and
        transitions from `num` alone as mstep would set them.  Both vectors must have been accumulated on this
        model.  Asynchronous"""
        _check(self.lib.ghmm_mstep_ebw(self.h, model.h, num.h, den.h, float(E)), self.lib)

    def score(self, model, corpus):
        out = np.empty(corpus.n_utt, dtype=np.float64)
        _check(self.lib.ghmm_score(self.h, model.h, corpus.h, _d(out)), self.lib)
        return out

    def score_batch(self, models, corpus):
        """RF:326-374 for a whole vocabulary: out[k, u] = log P(utterance u | model k)."""
        arr = (_vp * len(models))(*[m.h for m in models])
        out = np.empty((len(models), corpus.n_utt), dtype=np.float64)
        _check(self.lib.ghmm_score_batch(self.h, arr, len(models), corpus.h, _d(out)), self.lib)
        return out

    # ---- several feature streams (param_number P > 1)
    def estep_streams(self, models, corpora, stats):
        P = len(models)
        pm = (_vp * P)(*[m.h for m in models])
        pc = (_vp * P)(*[c.h for c in corpora])
        ps = (_vp * P)(*[s.h for s in stats])
        _check(self.lib.ghmm_estep_streams(self.h, pm, pc, P, ps), self.lib)

    def estep_log_streams(self, models, corpora, stats):
        """estep_log on several feature streams (ghmm_estep_log_streams)"""
        P = len(models)
        pm = (_vp * P)(*[m.h for m in models])
        pc = (_vp * P)(*[c.h for c in corpora])
        ps = (_vp * P)(*[s.h for s in stats])
        _check(self.lib.ghmm_estep_log_streams(self.h, pm, pc, P, ps), self.lib)

    def score_streams(self, models, corpora):
        P = len(models)
        pm = (_vp * P)(*[m.h for m in models])
        pc = (_vp * P)(*[c.h for c in corpora])
        out = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(self.lib.ghmm_score_streams(self.h, pm, pc, P, _d(out)), self.lib)
        return out

    # ---- several-stream vocabularies of diagonal models: vocab[k][p] = stream p of word k
    def viterbi_streams(self, models, corpora):
        """viterbi on the sum of the streams' log b: (path, score); fetch(BUF_B, (frames, N)) is that sum"""
        path = np.empty(corpora[0].frames, dtype=np.int32)
        score = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(self.lib.ghmm_viterbi_streams(self.h, self._stream_handles(models), self._stream_handles(corpora),
                                             len(models), path.ctypes.data_as(_ip), _d(score)), self.lib)
        return path, score

    def score_streams_batch(self, vocab, corpora):
        """out[k, u] = score_streams of word k, the vocabulary in one pass"""
        out = np.empty((len(vocab), corpora[0].n_utt), dtype=np.float64)
        _check(self.lib.ghmm_score_streams_batch(self.h, self._vocab_handles(vocab), len(vocab),
                                                 self._stream_handles(corpora), len(corpora), _d(out)), self.lib)
        return out

    def viterbi_streams_batch(self, vocab, corpora):
        """out[k, u] = viterbi_streams' score of word k, the vocabulary in one pass"""
        out = np.empty((len(vocab), corpora[0].n_utt), dtype=np.float64)
        _check(self.lib.ghmm_viterbi_streams_batch(self.h, self._vocab_handles(vocab), len(vocab),
                                                   self._stream_handles(corpora), len(corpora), _d(out)), self.lib)
        return out

    def recognise_streams(self, vocab, corpora):
        """(word[U], path[F], score[K, U]): every utterance's best word by Viterbi score (ties: the
        lowest word), that word's path over the utterance's frames, and the whole score table"""
        word = np.empty(corpora[0].n_utt, dtype=np.int32)
        path = np.empty(corpora[0].frames, dtype=np.int32)
        score = np.empty((len(vocab), corpora[0].n_utt), dtype=np.float64)
        _check(self.lib.ghmm_recognise_streams(self.h, self._vocab_handles(vocab), len(vocab),
                                               self._stream_handles(corpora), len(corpora),
                                               word.ctypes.data_as(_ip), path.ctypes.data_as(_ip), _d(score)),
               self.lib)
        return word, path, score

    def _connect(self, fn, vocab, corpora, penalty):
        F = corpora[0].frames
        word, path, begin = (np.empty(F, dtype=np.int32) for _ in range(3))
        score = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(fn(self.h, self._vocab_handles(vocab), len(vocab), self._stream_handles(corpora), len(corpora),
                  float(penalty), word.ctypes.data_as(_ip), path.ctypes.data_as(_ip), begin.ctypes.data_as(_ip),
                  _d(score)), self.lib)
        return word, path, begin, score

    def connect_streams(self, vocab, corpora, penalty=0.0):
        """(word[F], path[F], begin[F], score[U]): every utterance decoded as a string of the vocabulary's
        words by one Viterbi lattice over all of them; `penalty` is added at every word entry after the
        first.  begin is 1 on the first frame of every word instance (word_segments takes it apart)"""
        return self._connect(self.lib.ghmm_connect_streams, vocab, corpora, penalty)

    def connect_full_streams(self, vocab, corpora, penalty=0.0):
        """connect_streams for full-covariance words"""
        return self._connect(self.lib.ghmm_connect_full_streams, vocab, corpora, penalty)

    def _connect_grammar(self, fn, vocab, corpora, pair, start, fin):
        K, F = len(vocab), corpora[0].frames
        pair = np.ascontiguousarray(pair, dtype=np.float64)
        if pair.shape != (K, K):
            raise ValueError(f"pair has shape {pair.shape}, the vocabulary has {K} words")
        rows = []
        for name, a in (("start", start), ("fin", fin)):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
            if a is not None and a.shape != (K,):
                raise ValueError(f"{name} has shape {a.shape}, the vocabulary has {K} words")
            rows.append(a)
        word, path, begin = (np.empty(F, dtype=np.int32) for _ in range(3))
        score = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(fn(self.h, self._vocab_handles(vocab), K, self._stream_handles(corpora), len(corpora), _d(rows[0]),
                  _d(pair), _d(rows[1]), word.ctypes.data_as(_ip), path.ctypes.data_as(_ip),
                  begin.ctypes.data_as(_ip), _d(score)), self.lib)
        return word, path, begin, score

    def connect_grammar_streams(self, vocab, corpora, pair, start=None, fin=None):
        """connect_streams under a word-pair grammar, the same tuple (word_segments works on it):
        pair[w, k] = the log score of word k following word w, start[k] of word k opening the utterance,
        fin[k] of word k closing it (None: all 0); -inf forbids.  bigram_log estimates the three from
        transcripts"""
        return self._connect_grammar(self.lib.ghmm_connect_grammar_streams, vocab, corpora, pair, start, fin)

    def connect_grammar_full_streams(self, vocab, corpora, pair, start=None, fin=None):
        """connect_grammar_streams for full-covariance words"""
        return self._connect_grammar(self.lib.ghmm_connect_grammar_full_streams, vocab, corpora, pair, start, fin)

    def _grammar_post(self, fn, vocab, corpora, pair, start, fin, entries):
        K, F = len(vocab), corpora[0].frames
        pair = np.ascontiguousarray(pair, dtype=np.float64)
        if pair.shape != (K, K):
            raise ValueError(f"pair has shape {pair.shape}, the vocabulary has {K} words")
        rows = []
        for name, a in (("start", start), ("fin", fin)):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
            if a is not None and a.shape != (K,):
                raise ValueError(f"{name} has shape {a.shape}, the vocabulary has {K} words")
            rows.append(a)
        occ = np.empty((F, K), dtype=np.float64)
        ent = np.empty((F, K), dtype=np.float64) if entries else None
        loglik = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(fn(self.h, self._vocab_handles(vocab), K, self._stream_handles(corpora), len(corpora), _d(rows[0]),
                  _d(pair), _d(rows[1]), _d(occ), _d(ent), _d(loglik)), self.lib)
        return (occ, ent, loglik) if entries else (occ, loglik)

    def grammar_post_streams(self, vocab, corpora, pair, start=None, fin=None, entries=False):
        """word posteriors under connect_grammar_streams' grammar, by a log-domain forward-backward over its
        lattice: (occ[F, K], loglik[U]), occ[f, k] = the posterior that frame f lies in word k, loglik[u] =
        log P of utterance u summed over every word string the grammar allows; with entries (occ, ent,
        loglik), ent[f, k] = the posterior that an instance of word k begins at frame f.  An utterance whose
        log P is not finite has zero rows.  word_confidence turns occ into a confidence per decoded word;
        fetch(BUF_GAMMA, (frames, NS)) is the posterior per composite state"""
        return self._grammar_post(self.lib.ghmm_grammar_post_streams, vocab, corpora, pair, start, fin, entries)

    def grammar_post_full_streams(self, vocab, corpora, pair, start=None, fin=None, entries=False):
        """grammar_post_streams for full-covariance words"""
        return self._grammar_post(self.lib.ghmm_grammar_post_full_streams, vocab, corpora, pair, start, fin, entries)

    def _align(self, fn, vocab, corpora, transcripts):
        F, U = corpora[0].frames, corpora[0].n_utt
        if len(transcripts) != U:
            raise ValueError(f"{len(transcripts)} transcripts for {U} utterances")
        seq_off = np.zeros(U + 1, dtype=np.int32)
        seq_off[1:] = np.cumsum([len(t) for t in transcripts])
        seq = np.array([k for t in transcripts for k in t] + [0], dtype=np.int32)     # (never of size 0)
        word, path, begin = (np.empty(F, dtype=np.int32) for _ in range(3))
        score = np.empty(U, dtype=np.float64)
        _check(fn(self.h, self._vocab_handles(vocab), len(vocab), self._stream_handles(corpora), len(corpora),
                  seq.ctypes.data_as(_ip), seq_off.ctypes.data_as(_ip), word.ctypes.data_as(_ip),
                  path.ctypes.data_as(_ip), begin.ctypes.data_as(_ip), _d(score)), self.lib)
        return word, path, begin, score

    def align_streams(self, vocab, corpora, transcripts):
        """(word[F], path[F], begin[F], score[U]): every utterance aligned with its known transcript,
        transcripts[u] = the sequence of its words' indices into vocab.  The outputs have connect_streams'
        shape (word_segments takes them apart, cut_segments cuts the corpus at them); a score of -inf says
        the utterance is too short for its transcript, its frame entries then carry no meaning"""
        return self._align(self.lib.ghmm_align_streams, vocab, corpora, transcripts)

    def align_full_streams(self, vocab, corpora, transcripts):
        """align_streams for full-covariance words"""
        return self._align(self.lib.ghmm_align_full_streams, vocab, corpora, transcripts)

    def _estep_embed(self, fn, vocab, corpora, transcripts, stats):
        U = corpora[0].n_utt
        if len(transcripts) != U:
            raise ValueError(f"{len(transcripts)} transcripts for {U} utterances")
        seq_off = np.zeros(U + 1, dtype=np.int32)
        seq_off[1:] = np.cumsum([len(t) for t in transcripts])
        seq = np.array([k for t in transcripts for k in t] + [0], dtype=np.int32)     # (never of size 0)
        _check(fn(self.h, self._vocab_handles(vocab), len(vocab), self._stream_handles(corpora), len(corpora),
                  seq.ctypes.data_as(_ip), seq_off.ctypes.data_as(_ip), self._vocab_handles(stats)), self.lib)

    def estep_embed_streams(self, vocab, corpora, transcripts, stats):
        """the embedded Baum-Welch E-step: forward-backward over every utterance's transcript
        (transcripts[u] = the sequence of its words' indices into vocab), gamma and xi tied over the
        instances of a word; stats[k][p] (word k's stream-p shape) is overwritten, so that
        mstep(vocab[k][p], stats[k][p]) follows.  Asynchronous; every vector carries the summed log P
        and the utterance count.  fetch(BUF_GAMMA, (frames, NS)) is the tied gamma"""
        self._estep_embed(self.lib.ghmm_estep_embed_streams, vocab, corpora, transcripts, stats)

    def estep_embed_full_streams(self, vocab, corpora, transcripts, stats):
        """estep_embed_streams for full-covariance words: stats[k][p] is a stats_full vector of word k's
        stream-p shape, so that mstep_full or mstep_full_dev(vocab[k][p], stats[k][p]) follows"""
        self._estep_embed(self.lib.ghmm_estep_embed_full_streams, vocab, corpora, transcripts, stats)

    def estep_grammar_streams(self, vocab, corpora, pair, stats, start=None, fin=None):
        """the Baum-Welch E-step over grammar_post_streams' lattice, that is over EVERY word string the grammar
        (pair, start, fin: connect_grammar_streams') allows: stats[k][p] (word k's stream-p shape) is
        overwritten in estep_embed_streams' layout, so that mstep(vocab[k][p], stats[k][p]) follows.  The sums
        are normalised by the lattice's own log P_u (not estep_embed_streams' log Z_u); an utterance whose log P
        is not finite adds only that to the summed log P.  Asynchronous; fetch(BUF_GAMMA, (frames, NS)) and
        fetch(BUF_LOGLIK, (n_utt,)) are grammar_post_streams'"""
        K = len(vocab)
        pair = np.ascontiguousarray(pair, dtype=np.float64)
        if pair.shape != (K, K):
            raise ValueError(f"pair has shape {pair.shape}, the vocabulary has {K} words")
        rows = []
        for name, a in (("start", start), ("fin", fin)):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
            if a is not None and a.shape != (K,):
                raise ValueError(f"{name} has shape {a.shape}, the vocabulary has {K} words")
            rows.append(a)
        _check(self.lib.ghmm_estep_grammar_streams(self.h, self._vocab_handles(vocab), K,
                                                   self._stream_handles(corpora), len(corpora), _d(rows[0]),
                                                   _d(pair), _d(rows[1]), self._vocab_handles(stats)), self.lib)

    # ---- the forward score of diagonal models in the log domain
    def logscore(self, model, corpus, final_state=False):
        """log-domain forward score per utterance: LSE over the last frame's states, or the last
        state's alone with final_state (score's quantity); finite where score underflows; log b stays
        in the workspace (fetch(BUF_B, (frames, N)))"""
        out = np.empty(corpus.n_utt, dtype=np.float64)
        _check(self.lib.ghmm_logscore(self.h, model.h, corpus.h, int(bool(final_state)), _d(out)), self.lib)
        return out

    def logscore_batch(self, models, corpus, final_state=False):
        """out[k, u] = logscore of utterance u under model k, the vocabulary in one pass"""
        arr = (_vp * len(models))(*[m.h for m in models])
        out = np.empty((len(models), corpus.n_utt), dtype=np.float64)
        _check(self.lib.ghmm_logscore_batch(self.h, arr, len(models), corpus.h, int(bool(final_state)), _d(out)),
               self.lib)
        return out

    def logscore_streams(self, models, corpora, final_state=False):
        """logscore on the sum of the streams' log b"""
        out = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(self.lib.ghmm_logscore_streams(self.h, self._stream_handles(models), self._stream_handles(corpora),
                                              len(models), int(bool(final_state)), _d(out)), self.lib)
        return out

    def logscore_streams_batch(self, vocab, corpora, final_state=False):
        """out[k, u] = logscore_streams of word k, the vocabulary in one pass"""
        out = np.empty((len(vocab), corpora[0].n_utt), dtype=np.float64)
        _check(self.lib.ghmm_logscore_streams_batch(self.h, self._vocab_handles(vocab), len(vocab),
                                                    self._stream_handles(corpora), len(corpora),
                                                    int(bool(final_state)), _d(out)), self.lib)
        return out

    # ---- the full-covariance recogniser
    def full_model(self, hfm):
        return FullModel(self, hfm)

    def emission_full(self, fmodel, corpus):
        """b[F][N] into the workspace (fetch(BUF_B, (frames, N)))"""
        _check(self.lib.ghmm_emission_full(self.h, fmodel.h, corpus.h), self.lib)

    def score_full(self, fmodel, corpus):
        """RC's log P per utterance: -sum_t log c_t (no final-state term)"""
        out = np.empty(corpus.n_utt, dtype=np.float64)
        _check(self.lib.ghmm_score_full(self.h, fmodel.h, corpus.h, _d(out)), self.lib)
        return out

    def score_full_batch(self, fmodels, corpus):
        """RC:326-374 for a whole vocabulary: out[k, u] = log P(utterance u | model k)."""
        arr = (_vp * len(fmodels))(*[m.h for m in fmodels])
        out = np.empty((len(fmodels), corpus.n_utt), dtype=np.float64)
        _check(self.lib.ghmm_score_full_batch(self.h, arr, len(fmodels), corpus.h, _d(out)),
               self.lib)
        return out

    def viterbi_full(self, fmodel, corpus):
        """best path (state per frame) and its log score per utterance, ending in the last state;
        log b stays in the workspace (fetch(BUF_B, (frames, N)))"""
        path = np.empty(corpus.frames, dtype=np.int32)
        score = np.empty(corpus.n_utt, dtype=np.float64)
        _check(self.lib.ghmm_viterbi_full(self.h, fmodel.h, corpus.h, path.ctypes.data_as(_ip),
                                          _d(score)), self.lib)
        return path, score

    def viterbi_full_batch(self, fmodels, corpus):
        """out[k, u] = Viterbi log score of utterance u under model k (= viterbi_full's, bit for bit)"""
        arr = (_vp * len(fmodels))(*[m.h for m in fmodels])
        out = np.empty((len(fmodels), corpus.n_utt), dtype=np.float64)
        _check(self.lib.ghmm_viterbi_full_batch(self.h, arr, len(fmodels), corpus.h, _d(out)),
               self.lib)
        return out

    def logscore_full(self, fmodel, corpus, final_state=False):
        """log-domain forward score per utterance: LSE over the last frame's states, or the last
        state's alone with final_state; finite where score_full underflows; log b stays in the
        workspace (fetch(BUF_B, (frames, N)))"""
        out = np.empty(corpus.n_utt, dtype=np.float64)
        _check(self.lib.ghmm_logscore_full(self.h, fmodel.h, corpus.h, int(bool(final_state)), _d(out)),
               self.lib)
        return out

    def logscore_full_batch(self, fmodels, corpus, final_state=False):
        """out[k, u] = log-domain forward score of utterance u under model k (= logscore_full's, bit
        for bit)"""
        arr = (_vp * len(fmodels))(*[m.h for m in fmodels])
        out = np.empty((len(fmodels), corpus.n_utt), dtype=np.float64)
        _check(self.lib.ghmm_logscore_full_batch(self.h, arr, len(fmodels), corpus.h,
                                                 int(bool(final_state)), _d(out)), self.lib)
        return out

    # ---- the full-covariance trainer
    @staticmethod
    def init_model_full(X, lens, N, M):
        """TFF's initial model (host code, ghmm_init_model_full) as a HostFullModel"""
        return HostFullModel.init_from(X, lens, N, M)

    def estep_full(self, fmodel, corpus, stats):
        """TFF's E-step (ghmm_estep_full) into a stats_full vector; b / post / gamma stay in the
        workspace (fetch)"""
        _check(self.lib.ghmm_estep_full(self.h, fmodel.h, corpus.h, stats.h), self.lib)

    def estep_full_log(self, fmodel, corpus, stats):
        """the same E-step in the log domain (ghmm_estep_full_log): finite where estep_full's linear
        densities underflow; afterwards fetch(BUF_B) is log b, BUF_ALPHA / BUF_BETA the log lattices"""
        _check(self.lib.ghmm_estep_full_log(self.h, fmodel.h, corpus.h, stats.h), self.lib)

    def mstep_full(self, fmodel, stats):
        """TFF's M-step (ghmm_mstep_full: host numerics, then the model is set again)"""
        _check(self.lib.ghmm_mstep_full(self.h, fmodel.h, stats.h), self.lib)

    def mstep_full_dev(self, fmodel, stats):
        """the same M-step by HIP kernels on the stream (ghmm_mstep_full_dev): asynchronous, nothing
        is downloaded; the model's parameters equal mstep_full's bit for bit"""
        _check(self.lib.ghmm_mstep_full_dev(self.h, fmodel.h, stats.h), self.lib)

    # ---- the full-covariance calls on several feature streams (param_number P > 1)
    @staticmethod
    def _stream_handles(objs):
        return (_vp * len(objs))(*[o.h for o in objs])

    def estep_full_streams(self, fmodels, corpora, stats, log=False):
        """TFF's E-step on the product of the streams' densities (ghmm_estep_full_streams), `log`: in
        the log domain; stats[p] = stream p's stats_full vector; fetch(BUF_B) is the product (log:
        the sum of the streams' log b)"""
        _check(self.lib.ghmm_estep_full_streams(self.h, self._stream_handles(fmodels), self._stream_handles(corpora),
                                                len(fmodels), self._stream_handles(stats), int(bool(log))),
               self.lib)

    def score_full_streams(self, fmodels, corpora):
        """score_full on the product of the streams' densities"""
        out = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(self.lib.ghmm_score_full_streams(self.h, self._stream_handles(fmodels), self._stream_handles(corpora),
                                                len(fmodels), _d(out)), self.lib)
        return out

    def logscore_full_streams(self, fmodels, corpora, final_state=False):
        """logscore_full on the sum of the streams' log b"""
        out = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(self.lib.ghmm_logscore_full_streams(self.h, self._stream_handles(fmodels),
                                                   self._stream_handles(corpora), len(fmodels),
                                                   int(bool(final_state)), _d(out)), self.lib)
        return out

    # ---- several-stream vocabularies: vocab[k][p] = stream p of word k
    def viterbi_full_streams(self, fmodels, corpora):
        """viterbi_full on the sum of the streams' log b: (path, score)"""
        path = np.empty(corpora[0].frames, dtype=np.int32)
        score = np.empty(corpora[0].n_utt, dtype=np.float64)
        _check(self.lib.ghmm_viterbi_full_streams(self.h, self._stream_handles(fmodels),
                                                  self._stream_handles(corpora), len(fmodels),
                                                  path.ctypes.data_as(_ip), _d(score)), self.lib)
        return path, score

    @staticmethod
    def _vocab_handles(vocab):
        P = len(vocab[0])
        if any(len(w) != P for w in vocab):
            raise ValueError("every word of the vocabulary needs one model per stream")
        return (_vp * (len(vocab) * P))(*[m.h for w in vocab for m in w])

    def score_full_streams_batch(self, vocab, corpora):
        """out[k, u] = score_full_streams of word k (bit for bit), the vocabulary in one pass"""
        out = np.empty((len(vocab), corpora[0].n_utt), dtype=np.float64)
        _check(self.lib.ghmm_score_full_streams_batch(self.h, self._vocab_handles(vocab), len(vocab),
                                                      self._stream_handles(corpora), len(corpora), _d(out)),
               self.lib)
        return out

    def logscore_full_streams_batch(self, vocab, corpora, final_state=False):
        """out[k, u] = logscore_full_streams of word k (bit for bit), the vocabulary in one pass"""
        out = np.empty((len(vocab), corpora[0].n_utt), dtype=np.float64)
        _check(self.lib.ghmm_logscore_full_streams_batch(self.h, self._vocab_handles(vocab), len(vocab),
                                                         self._stream_handles(corpora), len(corpora),
                                                         int(bool(final_state)), _d(out)), self.lib)
        return out

    def viterbi_full_streams_batch(self, vocab, corpora):
        """out[k, u] = viterbi_full_streams' score of word k (bit for bit), the vocabulary in one pass"""
        out = np.empty((len(vocab), corpora[0].n_utt), dtype=np.float64)
        _check(self.lib.ghmm_viterbi_full_streams_batch(self.h, self._vocab_handles(vocab), len(vocab),
                                                        self._stream_handles(corpora), len(corpora), _d(out)),
               self.lib)
        return out

    def recognise_full_streams(self, vocab, corpora):
        """(word[U], path[F], score[K, U]): every utterance's best word by Viterbi score (ties: the
        lowest word), that word's path over the utterance's frames, and the whole score table"""
        word = np.empty(corpora[0].n_utt, dtype=np.int32)
        path = np.empty(corpora[0].frames, dtype=np.int32)
        score = np.empty((len(vocab), corpora[0].n_utt), dtype=np.float64)
        _check(self.lib.ghmm_recognise_full_streams(self.h, self._vocab_handles(vocab), len(vocab),
                                                    self._stream_handles(corpora), len(corpora),
                                                    word.ctypes.data_as(_ip), path.ctypes.data_as(_ip),
                                                    _d(score)), self.lib)
        return word, path, score

    def viterbi(self, model, corpus):
        path = np.empty(corpus.frames, dtype=np.int32)
        score = np.empty(corpus.n_utt, dtype=np.float64)
        _check(self.lib.ghmm_viterbi(self.h, model.h, corpus.h, path.ctypes.data_as(_ip),
                                     _d(score)), self.lib)
        return path, score


class Model:
    def __init__(self, ctx, hm):
        self.ctx, self.N, self.M, self.D = ctx, hm.N, hm.M, hm.D
        h = _vp()
        _check(ctx.lib.ghmm_model_create(ctx.h, hm.N, hm.M, hm.D, C.byref(h)), ctx.lib)
        self.h = h
        ctx._children.append(self)
        self.set(hm)

    def set(self, hm):
        _check(self.ctx.lib.ghmm_model_set(self.ctx.h, self.h, *(_d(x) for x in hm.arrays())),
               self.ctx.lib)

    def init_from(self, corpus, comm=None, fetch=True):
        """creating_initial_model (TF:732) on the device; returns the model as HostModel
        (fetch=False: leaves it on the device, nothing is downloaded).
        `comm`: the corpus is one rank's shard, the k-means sums are all-reduced."""
        _check(self.ctx.lib.ghmm_model_init_comm(self.ctx.h, self.h, corpus.h,
                                                 comm.h if comm is not None else None),
               self.ctx.lib)
        return self.get() if fetch else None

    def get(self):
        N, M, D = self.N, self.M, self.D
        A = np.empty((N, N)); c = np.empty((N, M)); mu = np.empty((N, M, D))
        iv = np.empty((N, M, D)); det = np.empty((N, M))
        _check(self.ctx.lib.ghmm_model_get(self.ctx.h, self.h, _d(A), _d(c), _d(mu), _d(iv),
                                           _d(det)), self.ctx.lib)
        return HostModel(A, c, mu, iv, det)

    def close(self):
        if self.h:
            self.ctx.lib.ghmm_model_destroy(self.ctx.h, self.h)
            self.h = None


class FullModel:
    """Device-resident full-covariance model (ghmm_fmodel)."""

    def __init__(self, ctx, hfm):
        self.ctx, self.N, self.M, self.D = ctx, hfm.N, hfm.M, hfm.D
        h = _vp()
        _check(ctx.lib.ghmm_fmodel_create(ctx.h, hfm.N, hfm.M, hfm.D, C.byref(h)), ctx.lib)
        self.h = h
        ctx._children.append(self)
        self.set(hfm)

    def set(self, hfm):
        _check(self.ctx.lib.ghmm_fmodel_set(self.ctx.h, self.h, *(_d(x) for x in hfm.arrays())),
               self.ctx.lib)

    def get(self):
        N, M, D = self.N, self.M, self.D
        A = np.empty((N, N)); c = np.empty((N, M)); mu = np.empty((N, M, D))
        ic = np.empty((N, M, D, D)); det = np.empty((N, M))
        _check(self.ctx.lib.ghmm_fmodel_get(self.ctx.h, self.h, _d(A), _d(c), _d(mu), _d(ic),
                                            _d(det)), self.ctx.lib)
        return HostFullModel(A, c, mu, ic, det)

    def init_from(self, corpus, comm=None, fetch=True):
        """creating_initial_model (TFF:731) on the device (ghmm_fmodel_init): asynchronous on the
        stream; returns the model as HostFullModel (fetch=False: leaves it on the device, nothing is
        downloaded or waited for).  `comm`: the corpus is one rank's shard, every pass's sums are
        all-reduced."""
        _check(self.ctx.lib.ghmm_fmodel_init(self.ctx.h, self.h, corpus.h,
                                             comm.h if comm is not None else None), self.ctx.lib)
        return self.get() if fetch else None

    def dims(self):
        n, m, d = C.c_int(), C.c_int(), C.c_int()
        _check(self.ctx.lib.ghmm_fmodel_dims(self.h, C.byref(n), C.byref(m), C.byref(d)), self.ctx.lib)
        return n.value, m.value, d.value

    def close(self):
        if self.h:
            self.ctx.lib.ghmm_fmodel_destroy(self.ctx.h, self.h)
            self.h = None


class Corpus:
    def __init__(self, ctx, X, lens, dev_ptr=None, D=None):
        self.ctx = ctx
        self.lens = np.ascontiguousarray(lens, dtype=np.int32)
        self.n_utt = len(self.lens)
        self.frames = int(self.lens.sum())
        h = _vp()
        lp = self.lens.ctypes.data_as(_ip)
        if dev_ptr is None:
            X = _f64(X)
            assert X.shape[0] == self.frames
            self.D = X.shape[1]
            _check(ctx.lib.ghmm_corpus_create(ctx.h, _d(X), lp, self.n_utt, self.D, C.byref(h)),
                   ctx.lib)
        else:
            self.D = D
            _check(ctx.lib.ghmm_corpus_wrap(ctx.h, _vp(dev_ptr), lp, self.n_utt, D, C.byref(h)),
                   ctx.lib)
        self.h = h
        ctx._children.append(self)

    def close(self):
        if self.h:
            self.ctx.lib.ghmm_corpus_destroy(self.ctx.h, self.h)
            self.h = None


class Comm:
    """One rank of an RCCL communicator (ghmm_comm_*): the statistics all-reduce in C."""

    def __init__(self, ctx, rank, world, id_bytes=None, path=None, timeout_s=120.0):
        self.ctx = ctx
        h = _vp()
        if path is not None:
            _check(ctx.lib.ghmm_comm_create_file(ctx.h, os.fsencode(path), rank, world, timeout_s,
                                                 C.byref(h)), ctx.lib)
        else:
            if id_bytes is None:
                buf = C.create_string_buffer(128)
                _check(ctx.lib.ghmm_comm_unique_id(buf), ctx.lib)
                id_bytes = buf.raw
            buf = C.create_string_buffer(id_bytes, 128)
            _check(ctx.lib.ghmm_comm_create(ctx.h, buf, rank, world, C.byref(h)), ctx.lib)
        self.h = h
        ctx._children.append(self)

    @property
    def rank(self):
        return self.ctx.lib.ghmm_comm_rank(self.h)

    @property
    def size(self):
        return self.ctx.lib.ghmm_comm_size(self.h)

    def close(self):
        if self.h:
            self.ctx.lib.ghmm_comm_destroy(self.h)
            self.h = None


class Stats:
    def __init__(self, ctx, N, M, D, dev_ptr=None, full=False):
        self.ctx, self.N, self.M, self.D, self.full = ctx, N, M, D, full
        if full:
            self.n = stats_len_full(N, M, D)
            assert ctx.lib.ghmm_stats_len_full(N, M, D) == self.n
        else:
            self.n = stats_len(N, M, D)
            assert ctx.lib.ghmm_stats_len(N, M, D) == self.n
        h = _vp()
        if full:
            assert dev_ptr is None, "a full-covariance statistics vector is always the library's own"
            _check(ctx.lib.ghmm_stats_create_full(ctx.h, N, M, D, C.byref(h)), ctx.lib)
        elif dev_ptr is None:
            _check(ctx.lib.ghmm_stats_create(ctx.h, N, M, D, C.byref(h)), ctx.lib)
        else:
            _check(ctx.lib.ghmm_stats_wrap(ctx.h, N, M, D, _vp(dev_ptr), C.byref(h)), ctx.lib)
        self.h = h
        ctx._children.append(self)

    def download(self):
        out = np.empty(self.n, dtype=np.float64)
        _check(self.ctx.lib.ghmm_stats_download(self.ctx.h, self.h, _d(out)), self.ctx.lib)
        return out

    def loglik(self):
        """(sum of log P, utterance count): the 16 bytes the stopping rule reads (TF:318-325)"""
        out = np.empty(2, dtype=np.float64)
        _check(self.ctx.lib.ghmm_stats_loglik(self.ctx.h, self.h, _d(out)), self.ctx.lib)
        return float(out[0]), float(out[1])

    def upload(self, v):
        v = _f64(v)
        assert v.size == self.n
        _check(self.ctx.lib.ghmm_stats_upload(self.ctx.h, self.h, _d(v)), self.ctx.lib)

    def close(self):
        if self.h:
            self.ctx.lib.ghmm_stats_destroy(self.ctx.h, self.h)
            self.h = None
