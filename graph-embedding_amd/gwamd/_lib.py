"""ctypes binding of libgraphwalk (include/graphwalk.h).

The shared library is built in-tree by graph-embedding_amd/build.py.  There is
no CPU fallback: if the library (or a GPU, for compute calls) is missing the
calls raise.

torch is imported first when it is installed: libtorch ships its own
libamdhip64.so.7, and loading it before libgraphwalk makes both share ONE HIP
runtime (so torch streams/pointers are valid handles for this library).
"""
import ctypes
import os

try:  # share torch's HIP runtime (see module docstring)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the library
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GW_LIB", os.path.join(_HERE, "libgraphwalk.so"))

GW_OK = 0
GW_ERR_INVALID = -1
GW_ERR_IO = -2
GW_ERR_PARSE = -3
GW_ERR_NOMEM = -4
GW_ERR_DEVICE = -5
GW_ERR_STATE = -6
GW_ERR_UNSUPPORTED = -7
GW_ERR_RANGE = -8
GW_ERR_KEY = -9
GW_ERR_ZERODIV = -10
GW_ERR_CAPACITY = -11
GW_ERR_INTERNAL = -12

SEM_NX_SIMPLE = 0
SEM_JAVA_MULTI = 1
SEM_JAVA_WGRAPH = 2
SEMANTICS = {"nx": SEM_NX_SIMPLE, "java": SEM_JAVA_MULTI, "wgraph": SEM_JAVA_WGRAPH}
N2V_REPLAY = 0
N2V_REJECTION = 1
N2V_BITSET = 2
N2V_AUTO = 3
TOPSIM_SINGLE_SAMPLE = 0
TOPSIM_ENUMERATE = 1
TOPSIM_SINGLE_RW = 2
DOUBLE_SAMPLE = 0
DOUBLE_DEV = 1
DOUBLE_RANDOM_WALK = 2


class GraphWalkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class DeviceError(GraphWalkError):
    pass


class CapacityError(GraphWalkError):
    pass


class StateError(GraphWalkError):
    pass


class UnsupportedError(GraphWalkError):
    pass


class GraphInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("nnz", ctypes.c_int64),
                ("max_degree", ctypes.c_int64), ("edge_alias_entries", ctypes.c_int64),
                ("semantics", ctypes.c_int32), ("directed", ctypes.c_int32),
                ("weighted", ctypes.c_int32), ("device", ctypes.c_int32),
                ("sampler_bytes", ctypes.c_int64), ("n2v_mode", ctypes.c_int32), ("listed", ctypes.c_int32)]


class Options(ctypes.Structure):
    """gw_options_t (per-handle tuning, include/graphwalk.h)."""
    _fields_ = [("table_budget_bytes", ctypes.c_int64), ("expected_steps", ctypes.c_int64),
                ("listed", ctypes.c_int32), ("simrank_hbm_row", ctypes.c_int32),
                ("host_chunk_bytes", ctypes.c_int64), ("topsim_part_shrink", ctypes.c_int32),
                ("simrank_window", ctypes.c_int32)]


class SgnsParams(ctypes.Structure):
    """gw_sgns_params_t (include/graphwalk.h); struct_size is filled in by default."""
    _fields_ = [("struct_size", ctypes.c_int32), ("dim", ctypes.c_int32), ("window", ctypes.c_int32),
                ("negative", ctypes.c_int32), ("epochs", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("alpha", ctypes.c_double), ("min_alpha", ctypes.c_double), ("sample", ctypes.c_double),
                ("seed", ctypes.c_uint64)]

    def __init__(self, dim=128, window=5, negative=5, epochs=5, alpha=0.025, min_alpha=0.0001, sample=1e-3, seed=0):
        super().__init__(ctypes.sizeof(SgnsParams), dim, window, negative, epochs, 0, alpha, min_alpha, sample, seed)


class SgnsStats(ctypes.Structure):
    """gw_sgns_stats_t."""
    _fields_ = [("tokens_kept", ctypes.c_int64), ("pairs", ctypes.c_int64), ("negatives", ctypes.c_int64),
                ("negatives_centre", ctypes.c_int64), ("targets_clipped", ctypes.c_int64)]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


DEEPSIM_FALLBACK_ROW_MIN = 0
DEEPSIM_FALLBACK_POSITION = 1


class DeepSimParams(ctypes.Structure):
    """gw_deepsim_params_t (include/graphwalk.h); struct_size is filled in by default."""
    _fields_ = [("struct_size", ctypes.c_int32), ("dim", ctypes.c_int32), ("window", ctypes.c_int32),
                ("batch", ctypes.c_int32), ("fallback", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("vertex_num", ctypes.c_int64), ("learning_rate", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("epsilon", ctypes.c_double), ("score_scale", ctypes.c_double),
                ("seed", ctypes.c_uint64)]

    def __init__(self, vertex_num=0, dim=128, window=10, batch=128, fallback=DEEPSIM_FALLBACK_ROW_MIN,
                 learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, score_scale=1.0, seed=0):
        super().__init__(ctypes.sizeof(DeepSimParams), dim, window, batch, fallback, 0, vertex_num, learning_rate,
                         beta1, beta2, epsilon, score_scale, seed)


class SdneParams(ctypes.Structure):
    """gw_sdne_params_t (include/graphwalk.h); struct_size is filled in by default; units = (u0, u1, u2, u3[, u4])."""
    _fields_ = [("struct_size", ctypes.c_int32), ("units", ctypes.c_int32 * 5), ("batch", ctypes.c_int32),
                ("shuffle", ctypes.c_int32), ("learning_rate", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("epsilon", ctypes.c_double), ("weight_decay", ctypes.c_double),
                ("kl_weight", ctypes.c_double), ("kl_target", ctypes.c_double), ("seed", ctypes.c_uint64),
                ("nonzero_weight", ctypes.c_double), ("first_order", ctypes.c_double)]

    def __init__(self, units=(0, 400, 100, 300), batch=100, learning_rate=0.01, beta1=0.9, beta2=0.999, epsilon=1e-8,
                 weight_decay=0.1, kl_weight=0.1, kl_target=0.005, seed=0, nonzero_weight=1.0, first_order=0.0,
                 shuffle=0):
        u = [int(x) for x in units]
        if len(u) == 4:
            u.append(u[0])
        if len(u) != 5:
            raise ValueError("units must be (u0, u1, u2, u3) or (u0, u1, u2, u3, u4)")
        super().__init__(ctypes.sizeof(SdneParams), (ctypes.c_int32 * 5)(*u), batch, int(shuffle), learning_rate,
                         beta1, beta2, epsilon, weight_decay, kl_weight, kl_target, seed, nonzero_weight, first_order)


OVR_CONST_NEG = 0
OVR_CONST_POS = 1
OVR_FITTED = 2
OVR_NOT_CONVERGED = 3


class OvrParams(ctypes.Structure):
    """gw_ovr_params_t (include/graphwalk.h); struct_size is filled in by default."""
    _fields_ = [("struct_size", ctypes.c_int32), ("dim", ctypes.c_int32), ("labels", ctypes.c_int32),
                ("max_newton", ctypes.c_int32), ("max_cg", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("C", ctypes.c_double), ("gtol", ctypes.c_double), ("seed", ctypes.c_uint64)]

    def __init__(self, labels=0, dim=128, max_newton=100, max_cg=200, C=1.0, gtol=1e-8, seed=0):
        super().__init__(ctypes.sizeof(OvrParams), dim, labels, max_newton, max_cg, 0, C, gtol, seed)


class OvrStats(ctypes.Structure):
    """gw_ovr_stats_t."""
    _fields_ = [("passes", ctypes.c_int64), ("fitted", ctypes.c_int32), ("constant", ctypes.c_int32),
                ("not_converged", ctypes.c_int32), ("newton_max", ctypes.c_int32)]


KNN_COSINE = 0
KNN_DOT = 1


class KnnParams(ctypes.Structure):
    """gw_knn_params_t (include/graphwalk.h); struct_size is filled in by default."""
    _fields_ = [("struct_size", ctypes.c_int32), ("dim", ctypes.c_int32), ("topk", ctypes.c_int32),
                ("metric", ctypes.c_int32)]

    def __init__(self, dim=128, topk=20, metric=KNN_COSINE):
        super().__init__(ctypes.sizeof(KnnParams), dim, topk, metric)


class NngParams(ctypes.Structure):
    """gw_nng_params_t (include/graphwalk.h); struct_size is filled in by default."""
    _fields_ = [("struct_size", ctypes.c_int32), ("dim", ctypes.c_int32), ("topk", ctypes.c_int32),
                ("include_self", ctypes.c_int32), ("heat_t", ctypes.c_double)]

    def __init__(self, dim=3, topk=10, include_self=1, heat_t=0.0):
        super().__init__(ctypes.sizeof(NngParams), dim, topk, int(include_self), heat_t)


GEO_SYM_UNION = 0
GEO_DIRECTED = 1


class GeoParams(ctypes.Structure):
    """gw_geo_params_t (include/graphwalk.h); struct_size is filled in by default."""
    _fields_ = [("struct_size", ctypes.c_int32), ("symmetrize", ctypes.c_int32), ("squared", ctypes.c_int32),
                ("delta", ctypes.c_double), ("round_cap", ctypes.c_int32)]

    def __init__(self, symmetrize=GEO_SYM_UNION, squared=0, delta=0.0, round_cap=0):
        super().__init__(ctypes.sizeof(GeoParams), symmetrize, int(squared), delta, int(round_cap))


class GeoStats(ctypes.Structure):
    """gw_geo_stats_t."""
    _fields_ = [("entries", ctypes.c_int64), ("components", ctypes.c_int64), ("main_component_size", ctypes.c_int64),
                ("rounds_max", ctypes.c_int64), ("relaxations", ctypes.c_int64), ("fallbacks", ctypes.c_int32)]


class LayoutParams(ctypes.Structure):
    """gw_layout_params_t (include/graphwalk.h); struct_size is filled in by default."""
    _fields_ = [("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def __init__(self):
        super().__init__(ctypes.sizeof(LayoutParams), 0)


LE_SYM_MEAN = 0
LE_SYM_MAX = 1
LE_CONVERGED = 0
LE_NOT_CONVERGED = 1


class LeParams(ctypes.Structure):
    """gw_le_params_t (include/graphwalk.h); struct_size is filled in by default; block 0 = dim + 32."""
    _fields_ = [("struct_size", ctypes.c_int32), ("dim", ctypes.c_int32), ("block", ctypes.c_int32),
                ("cheb_degree", ctypes.c_int32), ("max_iters", ctypes.c_int32), ("symmetrize", ctypes.c_int32),
                ("tol", ctypes.c_double), ("min_eigenvalue", ctypes.c_double), ("seed", ctypes.c_uint64),
                ("self_loops", ctypes.c_int32)]

    def __init__(self, dim=128, block=0, cheb_degree=20, max_iters=100, symmetrize=LE_SYM_MEAN, tol=1e-8,
                 min_eigenvalue=1e-5, seed=0, self_loops=0):
        super().__init__(ctypes.sizeof(LeParams), dim, block, cheb_degree, max_iters, symmetrize, tol, min_eigenvalue,
                         seed, int(self_loops))


class LeStats(ctypes.Structure):
    """gw_le_stats_t."""
    _fields_ = [("state", ctypes.c_int32), ("iters", ctypes.c_int32), ("applies", ctypes.c_int64),
                ("skipped", ctypes.c_int32), ("block_used", ctypes.c_int32), ("isolated", ctypes.c_int64),
                ("max_residual", ctypes.c_double)]


P = ctypes.c_void_p
I32 = ctypes.c_int32
I64 = ctypes.c_int64
U64 = ctypes.c_uint64
D = ctypes.c_double
CP = ctypes.c_char_p
PI32 = ctypes.POINTER(ctypes.c_int32)
PI64 = ctypes.POINTER(ctypes.c_int64)
PD = ctypes.POINTER(ctypes.c_double)
PP = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); mirrors include/graphwalk.h one to one
SIGNATURES = {
    "gw_version": (CP, []),
    "gw_last_error": (CP, [P]),
    "gw_strerror": (CP, [ctypes.c_int]),
    "gw_device_count": (ctypes.c_int, [PI32]),
    "gw_philox4x32": (ctypes.c_int, [ctypes.c_int, P, I64, P]),
    "gw_graph_load_edgelist": (ctypes.c_int, [CP, CP, ctypes.c_int, ctypes.c_int, ctypes.c_int, I64, PP]),
    "gw_graph_from_edges": (ctypes.c_int, [I64, P, P, P, ctypes.c_int, ctypes.c_int, I64, PP]),
    "gw_graph_from_csr": (ctypes.c_int, [I64, P, P, P, P, P, ctypes.c_int, ctypes.c_int, PP]),
    "gw_graph_rmat": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, D, D, D, U64, PP]),
    "gw_graph_rmat_java": (ctypes.c_int, [I64, I64, D, D, D, U64, PP]),
    "gw_graph_info": (ctypes.c_int, [P, ctypes.POINTER(GraphInfo)]),
    "gw_graph_set_options": (ctypes.c_int, [P, ctypes.POINTER(Options)]),
    "gw_graph_get_options": (ctypes.c_int, [P, ctypes.POINTER(Options)]),
    "gw_graph_export_csr": (ctypes.c_int, [P, P, P, P, P, P]),
    "gw_graph_export_weight_totals": (ctypes.c_int, [P, P]),
    "gw_graph_free": (ctypes.c_int, [P]),
    "gw_graph_to_device": (ctypes.c_int, [P, ctypes.c_int]),
    "gw_n2v_prepare": (ctypes.c_int, [P, D, D, ctypes.c_int]),
    "gw_n2v_export_alias": (ctypes.c_int, [P, P, P, P, P, P]),
    "gw_n2v_export_bitset": (ctypes.c_int, [P, P, P]),
    "gw_alias_setup": (ctypes.c_int, [ctypes.c_int, P, I64, P, P]),
    "gw_n2v_walks_replay": (ctypes.c_int, [P, ctypes.c_int, I64, P, P, I64, P, P, PI64]),
    "gw_n2v_walks": (ctypes.c_int, [P, ctypes.c_int, U64, I64, I64, ctypes.c_int, P, P, P, P]),
    "gw_n2v_walks_host": (ctypes.c_int, [P, ctypes.c_int, U64, I64, I64, ctypes.c_int, P, P, P]),
    "gw_topsim_host": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, D, U64, P, I64,
                                      ctypes.c_int, P, P, P, P]),
    "gw_topsim_prepare":(ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "gw_topsim_kernel": (ctypes.c_char_p, [P]),
    "gw_topsim_last_launches": (ctypes.c_int, [P]),
    "gw_topsim_kernel_attrs": (ctypes.c_int, [P, P, P, P]),
    "gw_topsim": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, D, U64, P, I64,
                                 ctypes.c_int, P, P, P, P]),
    "gw_topsim_dense": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, D, U64, P, I64,
                                       P, P, P]),
    "gw_topsim_sparse": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, D, U64, P, I64, I64,
                                        P, P, P, P, P, P, P]),
    "gw_topsim_write_text": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, D, U64, P, I64,
                                            ctypes.c_int, CP, CP, ctypes.c_int, P]),
    "gw_topsim_m": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, D, U64, P, I64,
                                   P, P, P, P, P]),
    "gw_topsim_m_host": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, D, U64, P,
                                        I64, P, P, P, P]),
    "gw_topsim_double": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, D, U64, P, P]),
    "gw_topsim_dev": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, D, U64, P, P, P]),
    "gw_double_random_walk": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, D, U64, P, P]),
    "gw_double_sim_host": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          D, U64, P, P]),
    "gw_select_fixed_max_pq": (ctypes.c_int, [P, I64, I64, ctypes.c_int, D, P]),
    "gw_format_java_double": (ctypes.c_int, [D, ctypes.c_char_p, I64]),
    "gw_simrank_naive": (ctypes.c_int, [P, D, ctypes.c_int, P, P]),
    "gw_simrank_naive_host": (ctypes.c_int, [P, D, ctypes.c_int, P]),
    "gw_simrank_weighted": (ctypes.c_int, [P, D, ctypes.c_int, P, P]),
    "gw_simrank_weighted_host": (ctypes.c_int, [P, D, ctypes.c_int, P]),
    "gw_simrank_weighted_ref": (ctypes.c_int, [P, D, ctypes.c_int, ctypes.c_int, P]),
    "gw_simrank_weighted_kernel_attrs": (ctypes.c_int, [P, P, P, P]),
    "gw_write_walks_text": (ctypes.c_int, [P, CP, P, P, I64, ctypes.c_int]),
    "gw_write_sim_text_dense": (ctypes.c_int, [CP, P, P, I64, I64, ctypes.c_int, CP, ctypes.c_int]),
    "gw_write_sim_text_topk": (ctypes.c_int, [CP, P, P, P, I64, ctypes.c_int, CP, ctypes.c_int]),
    "gw_write_sim_text_sparse": (ctypes.c_int, [CP, P, P, P, P, P, I64, I64, ctypes.c_int, CP, ctypes.c_int]),
    "gw_write_sim_text_cachemap": (ctypes.c_int, [CP, P, P, P, P, I64, ctypes.c_int, ctypes.c_int, CP]),
    "gw_sgns_create": (ctypes.c_int, [ctypes.c_int, I64, ctypes.POINTER(SgnsParams), PP]),
    "gw_sgns_free": (ctypes.c_int, [P]),
    "gw_sgns_last_error": (CP, [P]),
    "gw_sgns_build_vocab": (ctypes.c_int, [P, P, I64, ctypes.c_int]),
    "gw_sgns_train": (ctypes.c_int, [P, P, I64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(SgnsStats), P]),
    "gw_sgns_export": (ctypes.c_int, [P, P, P, P]),
    "gw_sgns_sampler_export": (ctypes.c_int, [P, P, P, P]),
    "gw_sgns_vectors_dev": (ctypes.c_int, [P, PP, PI64]),
    "gw_sgns_auto_concurrency_for": (ctypes.c_int, [P, I64, PI32]),
    "gw_sgns_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, PI32, PI32, PI32]),
    "gw_write_word2vec_text": (ctypes.c_int, [CP, P, P, P, I64, ctypes.c_int]),
    "gw_deepsim_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(DeepSimParams), PP]),
    "gw_deepsim_free": (ctypes.c_int, [P]),
    "gw_deepsim_last_error": (CP, [P]),
    "gw_deepsim_set_simrank": (ctypes.c_int, [P, P, P, ctypes.c_int]),
    "gw_deepsim_set_walks": (ctypes.c_int, [P, P, I64, ctypes.c_int, P, I64]),
    "gw_deepsim_train": (ctypes.c_int, [P, I64, I64, P, P]),
    "gw_deepsim_gradients": (ctypes.c_int, [P, I64, P, P, P, P]),
    "gw_deepsim_batch": (ctypes.c_int, [P, I64, P, P, P, P, P]),
    "gw_deepsim_export": (ctypes.c_int, [P, PP, PP, PP]),
    "gw_deepsim_vectors_dev": (ctypes.c_int, [P, PP, PI64]),
    "gw_deepsim_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(CP), PI32, PI32, PI32, PI32]),
    "gw_write_deepsim_text": (ctypes.c_int, [CP, P, I64, ctypes.c_int]),
    "gw_sdne_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(SdneParams), PP]),
    "gw_sdne_free": (ctypes.c_int, [P]),
    "gw_sdne_last_error": (CP, [P]),
    "gw_sdne_set_rows_dense": (ctypes.c_int, [P, P, I64, I64]),
    "gw_sdne_set_rows_csr": (ctypes.c_int, [P, P, P, P, I64]),
    "gw_sdne_train": (ctypes.c_int, [P, I64, I64, P, P]),
    "gw_sdne_gradients": (ctypes.c_int, [P, I64, PP]),
    "gw_sdne_batch_rows": (ctypes.c_int, [P, I64, P]),
    "gw_sdne_encode": (ctypes.c_int, [P, I64, I64, P]),
    "gw_sdne_export": (ctypes.c_int, [P, PP, PP, PP]),
    "gw_sdne_vectors_dev": (ctypes.c_int, [P, PP, PI64]),
    "gw_sdne_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(CP), PI32, PI32, PI32, PI32]),
    "gw_ovr_create": (ctypes.c_int, [ctypes.c_int, I64, ctypes.POINTER(OvrParams), PP]),
    "gw_ovr_free": (ctypes.c_int, [P]),
    "gw_ovr_last_error": (CP, [P]),
    "gw_ovr_set_features": (ctypes.c_int, [P, P, I64]),
    "gw_ovr_set_labels": (ctypes.c_int, [P, P, P]),
    "gw_ovr_order": (ctypes.c_int, [U64, U64, I64, P]),
    "gw_ovr_fit": (ctypes.c_int, [P, P, I64, ctypes.POINTER(OvrStats), P]),
    "gw_ovr_score": (ctypes.c_int, [P, P, I64, P, P]),
    "gw_ovr_decision": (ctypes.c_int, [P, P, I64, P]),
    "gw_ovr_export": (ctypes.c_int, [P, P, P, P, P]),
    "gw_ovr_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(CP), PI32, PI32, PI32, PI32]),
    "gw_knn_create": (ctypes.c_int, [ctypes.c_int, I64, ctypes.POINTER(KnnParams), PP]),
    "gw_knn_free": (ctypes.c_int, [P]),
    "gw_knn_last_error": (CP, [P]),
    "gw_knn_set_vectors": (ctypes.c_int, [P, P, I64]),
    "gw_knn_set_rows": (ctypes.c_int, [P, I64]),
    "gw_knn_query": (ctypes.c_int, [P, P, I64, P, P, P]),
    "gw_knn_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(CP), PI32, PI32, PI32, PI32]),
    "gw_knn_tiles": (ctypes.c_int, [P, PI32, PI32, PI32, PI32]),
    "gw_knn_fma_rate": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, PD]),
    "gw_topk_label_agreement": (ctypes.c_int, [P, I64, ctypes.c_int, P, P, P, I64, P]),
    "gw_nng_create": (ctypes.c_int, [ctypes.c_int, I64, ctypes.POINTER(NngParams), PP]),
    "gw_nng_free": (ctypes.c_int, [P]),
    "gw_nng_last_error": (CP, [P]),
    "gw_nng_set_vectors": (ctypes.c_int, [P, P, I64]),
    "gw_nng_set_rows": (ctypes.c_int, [P, I64]),
    "gw_nng_query": (ctypes.c_int, [P, P, I64, P, P, P, P]),
    "gw_nng_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(CP), PI32, PI32, PI32, PI32]),
    "gw_nng_tiles": (ctypes.c_int, [P, PI32, PI32, PI32, PI32]),
    "gw_geo_create": (ctypes.c_int, [ctypes.c_int, I64, ctypes.POINTER(GeoParams), PP]),
    "gw_geo_free": (ctypes.c_int, [P]),
    "gw_geo_last_error": (CP, [P]),
    "gw_geo_set_rows": (ctypes.c_int, [P, P, P, ctypes.c_int]),
    "gw_geo_set_csr": (ctypes.c_int, [P, P, P, P]),
    "gw_geo_components": (ctypes.c_int, [P, P, PI32]),
    "gw_geo_query": (ctypes.c_int, [P, P, I64, P, I64, P]),
    "gw_geo_stats": (ctypes.c_int, [P, ctypes.POINTER(GeoStats)]),
    "gw_geo_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(CP), PI32, PI32, PI32, PI32]),
    "gw_geo_tiles": (ctypes.c_int, [P, PI32, PI32, PI32]),
    "gw_layout_create": (ctypes.c_int, [ctypes.c_int, I64, ctypes.c_int, ctypes.POINTER(LayoutParams), PP]),
    "gw_layout_free": (ctypes.c_int, [P]),
    "gw_layout_last_error": (CP, [P]),
    "gw_layout_set_csr": (ctypes.c_int, [P, P, P, P]),
    "gw_layout_set_rows": (ctypes.c_int, [P, P, P, ctypes.c_int]),
    "gw_layout_set_fixed": (ctypes.c_int, [P, P, I64]),
    "gw_layout_run": (ctypes.c_int, [P, P, ctypes.c_double, ctypes.c_int32, ctypes.c_double, P, PI32]),
    "gw_layout_step": (ctypes.c_int, [P, P, ctypes.c_double, ctypes.c_double, P, P, P]),
    "gw_layout_rescale": (ctypes.c_int, [P, P, ctypes.c_double, P, P]),
    "gw_layout_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(CP), PI32, PI32, PI32, PI32]),
    "gw_layout_tiles": (ctypes.c_int, [P, PI32, PI32, PI32, PI32]),
    "gw_le_create": (ctypes.c_int, [ctypes.c_int, I64, ctypes.POINTER(LeParams), PP]),
    "gw_le_free": (ctypes.c_int, [P]),
    "gw_le_last_error": (CP, [P]),
    "gw_le_set_rows": (ctypes.c_int, [P, P, P, ctypes.c_int]),
    "gw_le_set_csr": (ctypes.c_int, [P, P, P, P]),
    "gw_le_solve": (ctypes.c_int, [P, ctypes.POINTER(LeStats), P]),
    "gw_le_export": (ctypes.c_int, [P, P, P, P]),
    "gw_le_vectors_dev": (ctypes.c_int, [P, PP, PI64]),
    "gw_le_apply": (ctypes.c_int, [P, P, P, ctypes.c_int]),
    "gw_le_tiles": (ctypes.c_int, [P, PI32, PI32, PI32]),
    "gw_le_kernel_attrs": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(CP), PI32, PI32, PI32, PI32]),
    "gw_le_time_kernel": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, PD]),
    "gw_comm_unique_id": (ctypes.c_int, [P]),
    "gw_comm_init": (ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, PP]),
    "gw_comm_allgather": (ctypes.c_int, [P, P, P, I64, ctypes.c_int, P]),
    "gw_comm_free": (ctypes.c_int, [P]),
    "gw_comm_last_error": (CP, [P]),
}

_lib = None


def lib():
    """Load libgraphwalk.so (raises ImportError when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"libgraphwalk.so not found at {LIB_PATH}: run `python graph-embedding_amd/build.py` "
                "(there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc, handle=None, sgns=None, deepsim=None, ovr=None, knn=None, le=None, sdne=None, nng=None, geo=None,
          layout=None):
    """Raise for a failing status; `handle` a gw_graph, `sgns` a gw_sgns, `deepsim` a gw_deepsim or True for a
    handle-less gw_deepsim call, `ovr`, `knn`, `le`, `sdne`, `nng` and `geo` likewise for gw_ovr, gw_knn, gw_le, gw_sdne,
    gw_nng and gw_geo, and `layout` for gw_layout (for the message)."""
    if rc == GW_OK:
        return
    L = lib()
    if layout is not None:
        msg = L.gw_layout_last_error(None if layout is True else layout)
    elif geo is not None:
        msg = L.gw_geo_last_error(None if geo is True else geo)
    elif nng is not None:
        msg = L.gw_nng_last_error(None if nng is True else nng)
    elif sdne is not None:
        msg = L.gw_sdne_last_error(None if sdne is True else sdne)
    elif le is not None:
        msg = L.gw_le_last_error(None if le is True else le)
    elif knn is not None:
        msg = L.gw_knn_last_error(None if knn is True else knn)
    elif ovr is not None:
        msg = L.gw_ovr_last_error(None if ovr is True else ovr)
    elif deepsim is not None:
        msg = L.gw_deepsim_last_error(None if deepsim is True else deepsim)
    else:
        msg = L.gw_sgns_last_error(sgns) if sgns is not None else L.gw_last_error(handle)
    msg = msg.decode(errors="replace")
    if rc == GW_ERR_INVALID:
        raise ValueError(msg)
    if rc == GW_ERR_IO:
        raise OSError(msg)
    if rc in (GW_ERR_PARSE,):
        raise ValueError(f"parse error: {msg}")
    if rc == GW_ERR_NOMEM:
        raise MemoryError(msg)
    if rc == GW_ERR_DEVICE:
        raise DeviceError(rc, msg)
    if rc == GW_ERR_STATE:
        raise StateError(rc, msg)
    if rc == GW_ERR_UNSUPPORTED:
        raise UnsupportedError(rc, msg)
    if rc == GW_ERR_RANGE:
        raise IndexError(msg)
    if rc == GW_ERR_KEY:
        raise KeyError(msg)
    if rc == GW_ERR_ZERODIV:
        raise ZeroDivisionError(msg)
    if rc == GW_ERR_CAPACITY:
        raise CapacityError(rc, msg)
    raise GraphWalkError(rc, msg)


def ptr(a):
    """Raw address of a numpy array / torch tensor / None."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return ctypes.c_void_p(a.data_ptr())
    return ctypes.c_void_p(a.ctypes.data)


def device_count():
    c = ctypes.c_int32(0)
    rc = lib().gw_device_count(ctypes.byref(c))
    return c.value if rc == GW_OK else 0
