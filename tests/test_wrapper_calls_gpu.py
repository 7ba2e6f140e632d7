"""The library calls behind every public wrapper of sigchain, utils, graph_utils, partition, nullmodel
and surrogate (with their numpy facades), as literals recorded from the commit before their argument
handling moved into nremmodfc_amd/_args.py: the first three before _args.py existed, the seeded three
before its seeded-run helpers did.

A fixture puts a proxy in the place of _lib.lib(): it forwards every call to libwcsde.so and records the
entry's name with every scalar argument, "p" or None for every pointer (never its value), the field
values of a struct passed by reference and the values of a ctypes array.  Each case calls one public
wrapper on the smallest input that reaches a branch; PLAN holds what the proxy recorded for it: the
same entries in the same order with the same scalars (ws_bytes among them: the library chunks by it)
and the same NULL pointers.  The cases return what the wrapper returned, so that a script can compare
their results between two commits bit for bit.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from nremmodfc_amd import (_lib, graph_utils as gu, nullmodel as nm, nullmodel_np as nmn, partition as pt,
                          partition_np as ptn, sigchain as sc, surrogate as sg, surrogate_np as sgn, utils as ut)

pytestmark = pytest.mark.gpu


def _plain(arg, ctype):
    if ctype is ctypes.c_void_p:
        return None if arg is None else "p"
    if isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer):
        if hasattr(arg, "_obj"):                      # byref(struct)
            s = arg._obj
            return {f: (list(v) if isinstance(v, ctypes.Array) else v)
                    for f, v in ((f, getattr(s, f)) for f, _ in s._fields_)}
        return None if arg is None else list(arg)     # a ctypes array
    return arg


class Recorder:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            assert len(args) == len(fn.argtypes)
            self.calls.append((name,) + tuple(_plain(a, t) for a, t in zip(args, fn.argtypes)))
            return fn(*args)
        return call


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def rand(dev, seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape)).to(dev)


def nrand(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape)


def weights(dev, seed, *shape):
    """Symmetric non-negative weights with a zero diagonal, [N][N] or [B][N][N]."""
    w = rand(dev, seed, *shape).abs()
    w = (w + w.transpose(-1, -2)) / 2
    w.diagonal(dim1=-2, dim2=-1).zero_()
    return w.contiguous()


def nweights(seed, *shape):
    w = np.abs(nrand(seed, *shape))
    w = (w + np.swapaxes(w, -1, -2)) / 2
    w[..., np.arange(shape[-1]), np.arange(shape[-1])] = 0
    return w


def phasors(dev, seed, *shape):
    th = rand(dev, seed, *shape)
    return torch.stack((torch.cos(th), torch.sin(th)), dim=-1).contiguous()


def labels(dev, seed, k, *shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(-1, k, shape).astype(np.int32)).to(dev)


def fc_stack(dev, seed, B, N):
    x = rand(dev, seed, B, N, N)
    return ((x + x.transpose(1, 2)) / 2).contiguous()


def _envelope_long_explicit(d):
    need = _lib.lib().wc_hilbert_envelope_workspace_size(2, 2048, 0)
    return sc.hilbert_envelope(rand(d, 4, 2048, 2), 0, ws_bytes=need + 4096)


def _bold_stream(d):
    bs = sc.BoldStream(2, sc.NEQ + 16, device=d)
    ring = torch.zeros(2 * 4000, dtype=torch.float32, device=d)
    bs.feed(rand(d, 60, 1000 * 2).float(), 1000, copy=ring, copy_ld=4000, copy_offset=1000)
    bs.feed(rand(d, 61, 1016, 2))
    return bs.finish(), ring


def _welch_accumulator(d):
    wa = sc.WelchAccumulator(1, 1, d)
    ring = rand(d, 62, 4000).float()
    wa.accumulate(ring, 4000, 1000, 4, 0)
    wa.accumulate(ring, 4000, 1000, 4, 2000)
    return wa.peak(want_psd=True)


def _kmeans_update(d):
    x, cent = rand(d, 40, 8, 2), rand(d, 41, 2, 2)
    lab, _ = sc.kmeans_assign(x, cent)
    return sc.kmeans_update(x, lab, cent), sc.kmeans_update(x, lab, cent, "sqeuclidean", ws_bytes=1 << 16)


def _phase_conn_aec97(d):
    return sc.phase_connectivity_from(phasors(d, 50, 16, 1, 97), rand(d, 51, 16, 1, 97).abs() + 0.1, ("aec",))


CI3 = np.array([[0, 1, 0, 1, 1], [1, 1, 0, 0, 1], [0, 0, 0, 1, 1]])
U64 = [0, 2 ** 64 - 1]                               # the second seed is negative in the int64 view that is uploaded
CI6 = [0, 0, 0, 1, 1, 1]


def signed(dev, seed, *shape):
    """Exactly symmetric weights of both signs with a zero diagonal, [N][N] or [B][N][N]."""
    x = rand(dev, seed, *shape)
    x = (x + x.transpose(-1, -2)) / 2
    x.diagonal(dim1=-2, dim2=-1).zero_()
    return x.contiguous()


def nsigned(seed, *shape):
    return signed("cpu", seed, *shape).numpy()


def cliques(dev, B=None):
    """The agreement of two 3-cliques, N = 6: every run finds them, a consensus in one iteration."""
    D = torch.block_diag(torch.ones(3, 3), torch.ones(3, 3)).double().fill_diagonal_(0).to(dev)
    return D if B is None else D.expand(B, 6, 6).contiguous()

CASES = {
    "hilbert_phase_8192": lambda d: sc.hilbert_phase(rand(d, 1, 8192, 2)),
    "hilbert_phase_8193": lambda d: sc.hilbert_phase(rand(d, 2, 8193, 2)),
    "hilbert_phase_long_explicit": lambda d: sc.hilbert_phase_long(rand(d, 2, 100, 2), ws_bytes=1 << 22),
    "hilbert_envelope_2047": lambda d: sc.hilbert_envelope(rand(d, 3, 2047, 2)),
    "hilbert_envelope_2048": lambda d: sc.hilbert_envelope(rand(d, 4, 2048, 2)),
    "hilbert_envelope_2047_ws_below_min": lambda d: sc.hilbert_envelope(rand(d, 3, 2047, 2), 0, ws_bytes=8),
    "hilbert_envelope_2048_explicit": _envelope_long_explicit,
    "hilbert_envelope_method1": lambda d: sc.hilbert_envelope(rand(d, 4, 2048, 2), 1),
    "hilbert_envelope_method2": lambda d: sc.hilbert_envelope(rand(d, 3, 100, 2), 2),
    "fc_metrics_96_K0": lambda d: sc.fc_metrics(rand(d, 5, 8, 2 * 96), 2, 96),
    "fc_metrics_96_K1": lambda d: sc.fc_metrics(rand(d, 5, 8, 2, 96), 2, 96, empfc=nrand(6, 1, 96, 96), want_fc=True),
    "fc_metrics_97_K0": lambda d: sc.fc_metrics(rand(d, 7, 8, 2 * 97), 2, 97, want_fc=True),
    "fc_metrics_97_K1_no_kuramoto": lambda d: sc.fc_metrics(rand(d, 7, 8, 2 * 97), 2, 97, empfc=nrand(8, 1, 97, 97),
                                                            kuramoto=False),
    "fc_metrics_fc_in": lambda d: sc.fc_metrics(fc_in=fc_stack(d, 9, 2, 8), empfc=nrand(10, 2, 8, 8), data_range=2.0),
    "hma_96": lambda d: sc.hma(fc_stack(d, 11, 2, 96)),
    "hma_96_clus_num": lambda d: sc.hma(fc_stack(d, 11, 2, 96), want_clus_num=True),
    "hma_2d": lambda d: sc.hma(fc_stack(d, 11, 1, 5)[0]),
    "hma_97": lambda d: sc.hma(fc_stack(d, 12, 2, 97)),
    "hma_97_clus_num": lambda d: sc.hma(fc_stack(d, 12, 2, 97), want_clus_num=True),
    "hma_97_B65": lambda d: sc.hma(fc_stack(d, 13, 65, 97)),
    "hma_97_B65_clus_num": lambda d: sc.hma(fc_stack(d, 13, 65, 97), want_clus_num=True),
    "graph_measures_dist": lambda d: sc.graph_measures(weights(d, 14, 3, 5, 5), ("dist",)),
    "graph_measures_degrees": lambda d: sc.graph_measures(weights(d, 14, 3, 5, 5), ("degrees",)),
    "graph_measures_all": lambda d: sc.graph_measures(weights(d, 14, 3, 5, 5)),
    "graph_measures_paths_lengths": lambda d: sc.graph_measures(weights(d, 14, 3, 5, 5), ["radius", "ecc", "radius"],
                                                                lengths=True, include_infinite=False),
    "graph_measures_N2_2d": lambda d: sc.graph_measures(weights(d, 15, 2, 2)),
    "graph_measures_N2_3d": lambda d: sc.graph_measures(weights(d, 15, 1, 2, 2)),
    "graph_betweenness": lambda d: sc.graph_betweenness(weights(d, 14, 3, 5, 5)),
    "graph_betweenness_2d_lengths": lambda d: sc.graph_betweenness(weights(d, 14, 5, 5), lengths=True),
    "graph_module_measures_ci_1d": lambda d: sc.graph_module_measures(
        weights(d, 14, 3, 5, 5), torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32, device=d)),
    "graph_module_measures_ci_2d": lambda d: sc.graph_module_measures(
        weights(d, 14, 3, 5, 5), torch.tensor(CI3, dtype=torch.int32, device=d), ("zscore",), degree="in", zflag=3,
        gamma=1.5, n_modules=2),
    "graph_module_measures_2d": lambda d: sc.graph_module_measures(
        weights(d, 14, 5, 5), torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32, device=d), "modularity"),
    "graph_louvain_seed_int": lambda d: sc.graph_louvain(weights(d, 16, 3, 3), seeds=3),
    "graph_louvain_seeds_list_info": lambda d: sc.graph_louvain(weights(d, 16, 2, 3, 3), seeds=[1, 2], gamma=0.9,
                                                                ci=[0, 0, 1], want_info=True),
    "graph_louvain_potts": lambda d: sc.graph_louvain((weights(d, 16, 3, 3) > 0.3).double(), objective="potts"),
    "graph_louvain_objective_tensor": lambda d: sc.graph_louvain(weights(d, 16, 3, 3), seeds=[5],
                                                                 objective=weights(d, 17, 3, 3) - 0.2),
    "graph_agreement": lambda d: sc.graph_agreement(labels(d, 18, 3, 2, 4, 5).abs()),
    "graph_agreement_2d": lambda d: sc.graph_agreement(labels(d, 18, 3, 4, 5).abs()),
    "graph_consensus_matrix": lambda d: sc.graph_consensus_matrix(weights(d, 19, 2, 5, 5), reps=2),
    "graph_consensus_matrix_seeds": lambda d: sc.graph_consensus_matrix(weights(d, 19, 5, 5), reps=2, tau=0.6,
                                                                        seeds=[7, 8]),
    "fcd_corr": lambda d: sc.fcd(rand(d, 20, 12, 3, 3), 4),
    "fcd_corr_explicit_ws": lambda d: sc.fcd(rand(d, 20, 12, 3, 3), 4, 2, want_windows=True, ws_bytes=1 << 16),
    "fcd_corr_2d": lambda d: sc.fcd(rand(d, 20, 12, 3), 4, want_windows=True),
    "fcd_phase": lambda d: sc.fcd(rand(d, 20, 12, 3, 3), method="phase", trim=1),
    "fcd_phase_2d": lambda d: sc.fcd(rand(d, 20, 12, 3), method="phase"),
    "fcd_from_phasors": lambda d: sc.fcd_from_phasors(phasors(d, 21, 6, 2, 3)),
    "fcd_from_phasors_3d": lambda d: sc.fcd_from_phasors(phasors(d, 21, 6, 3)),
    "fcd_ks": lambda d: sc.fcd_ks(sc.fcd(rand(d, 20, 12, 3, 3), 4), nrand(22, 7)),
    "leida": lambda d: sc.leida(rand(d, 23, 12, 2, 3), trim=1),
    "leida_2d": lambda d: sc.leida(rand(d, 23, 12, 3)),
    "leida_from_phasors": lambda d: sc.leida_from_phasors(phasors(d, 24, 6, 2, 3)),
    "leida_from_phasors_offset": lambda d: sc.leida_from_phasors(phasors(d, 24, 7, 3)[1:]),
    "kmeans_assign": lambda d: sc.kmeans_assign(rand(d, 25, 4, 2, 3), rand(d, 26, 2, 3), "sqeuclidean"),
    "kmeans_update": _kmeans_update,
    "kmeans_k": lambda d: sc.kmeans(rand(d, 40, 8, 2), 2, max_iter=1),
    "kmeans_init": lambda d: sc.kmeans(rand(d, 40, 4, 2, 2), rand(d, 41, 2, 2), "sqeuclidean", max_iter=2),
    "state_stats": lambda d: sc.state_stats(labels(d, 27, 3, 20, 2), 3),
    "state_stats_1d": lambda d: sc.state_stats(labels(d, 27, 3, 20), 3),
    "leida_states": lambda d: sc.leida_states(rand(d, 28, 6, 2, 3), rand(d, 29, 2, 3)),
    "leida_states_2d": lambda d: sc.leida_states(rand(d, 28, 6, 3), rand(d, 29, 2, 3), "sqeuclidean"),
    "state_kl": lambda d: sc.state_kl(rand(d, 30, 2, 3).abs(), [0.2, 0.3, 0.5]),
    "welch": lambda d: sc.welch(rand(d, 31, 64, 3), nperseg=8),
    "welch_3d_explicit_ws": lambda d: sc.welch(rand(d, 31, 64, 1, 3), 2.0, np.hanning(8), noverlap=2, detrend=False,
                                               scaling="spectrum", ws_bytes=1 << 20),
    "csd_matrix": lambda d: sc.csd(rand(d, 31, 64, 3), nperseg=8),
    "csd_pairs": lambda d: sc.csd(rand(d, 31, 64, 3), rand(d, 32, 64, 3), nperseg=8, ws_bytes=1 << 20),
    "coherence_matrix": lambda d: sc.coherence(rand(d, 31, 64, 3), nperseg=8),
    "coherence_pairs": lambda d: sc.coherence(rand(d, 31, 64, 3), rand(d, 32, 64, 3), nperseg=8),
    "spectrogram": lambda d: sc.spectrogram(rand(d, 31, 64, 3), nperseg=8),
    "spectrogram_3d_complex": lambda d: sc.spectrogram(rand(d, 31, 64, 1, 3), nperseg=8, noverlap=4, mode="complex"),
    "phase_connectivity_from_all": lambda d: sc.phase_connectivity_from(phasors(d, 33, 16, 2, 3),
                                                                        rand(d, 34, 16, 2, 3).abs()),
    "phase_connectivity_from_plv_3d": lambda d: sc.phase_connectivity_from(phasors(d, 33, 16, 3), None, "plv",
                                                                           ws_bytes=1 << 16),
    "phase_connectivity_from_aec_N1": lambda d: sc.phase_connectivity_from(phasors(d, 33, 16, 1),
                                                                           rand(d, 34, 16, 1).abs(), "aec"),
    "phase_connectivity_from_aec_97": _phase_conn_aec97,
    "phase_connectivity": lambda d: sc.phase_connectivity(rand(d, 35, 16, 2, 3)),
    "phase_connectivity_pli": lambda d: sc.phase_connectivity(rand(d, 35, 16, 3), ("pli", "plv", "pli")),
    "filtfilt": lambda d: sc.filtfilt([0.2, 0.3], [1.0, -0.5], rand(d, 36, 30, 2, 2)),
    "envelope": lambda d: sc.envelope(rand(d, 37, 60, 2)),
    "envelope_fcut": lambda d: sc.envelope(rand(d, 37, 60, 1, 2), 0.002, (8, 13), fcut=2.0),
    "kuramoto": lambda d: sc.kuramoto(rand(d, 38, 16, 6), B=2),
    "corrcoef": lambda d: sc.corrcoef(rand(d, 39, 16, 2, 3), 2, 3),
    "sim_bold": lambda d: sc.sim_bold(rand(d, 42, 2016, 1, 2)),
    "welch_peak": lambda d: sc.welch_peak(rand(d, 43, 8000, 1, 1), want_psd=True),
    "bold_stream": _bold_stream,
    "welch_accumulator": _welch_accumulator,
    # ---- partition, nullmodel, surrogate ----
    "louvain_sign_seeds_u64_info": lambda d: pt.graph_louvain_sign(signed(d, 60, 2, 6, 6), seeds=U64, want_info=True),
    "louvain_sign_seed_int_2d": lambda d: pt.graph_louvain_sign(signed(d, 60, 6, 6), seeds=3, gamma=0.9, qtype="neg"),
    "louvain_sign_one_slot": lambda d: pt.graph_louvain_sign(signed(d, 60, 2, 6, 6), seeds=[1, 2], qtype="smp",
                                                             ws_bytes=pt.louvain_sign_slot_bytes(6)),
    "graph_consensus": lambda d: pt.graph_consensus(cliques(d), 0.5, reps=2, max_iter=2),
    "graph_consensus_batch_seeds": lambda d: pt.graph_consensus(
        torch.stack([cliques(d), weights(d, 61, 6, 6).clamp(max=1.0)]), 0.3, reps=2, seeds=[2 ** 64 - 1, 5], max_iter=2),
    "graph_rewire_N4": lambda d: nm.graph_rewire(signed(d, 62, 4, 4)),
    "graph_rewire_N5_info_one_slot": lambda d: nm.graph_rewire(signed(d, 62, 2, 5, 5), bin_swaps=3, seeds=U64, want_info=True,
                                                               ws_bytes=nm.null_model_slot_bytes(5)),
    "graph_null_model_N4": lambda d: nm.graph_null_model(signed(d, 63, 4, 4)),
    "graph_null_model_N5_stats_one_slot": lambda d: nm.graph_null_model(
        signed(d, 63, 2, 5, 5), seeds=U64, bin_swaps=2, wei_freq=0.5, negative="reference", want_stats=True,
        ws_bytes=nm.null_model_slot_bytes(5)),
    "graph_null_model_sorted_once": lambda d: nm.graph_null_model(signed(d, 63, 5, 5), seeds=[4], wei_freq=0,
                                                                  want_stats=True),
    "participation_norm_chunks": lambda d: nm.participation_norm(signed(d, 64, 2, 6, 6), CI6, reps=3,
                                                                 max_bytes=8 * 2 * 6 * 6),
    "participation_norm_2d_seeds": lambda d: nm.participation_norm(
        signed(d, 64, 6, 6), torch.tensor(CI6, device=d), reps=2, seeds=[5, 6], bin_swaps=1, wei_freq=1, negative="reference"),
    "surrogate_fc": lambda d: sg.surrogate_fc(rand(d, 65, 4, 2), [1, 2]),
    "surrogate_fc_3d_u64": lambda d: sg.surrogate_fc(rand(d, 65, 4, 2, 2), U64),
    "fc_surrogate_test_chunks": lambda d: sg.fc_surrogate_test(rand(d, 66, 8, 3, 3), surr_number=2,
                                                               ws_bytes=sg.surrogate_slab_bytes(3, 2)),
    "fc_surrogate_test_2d_stats": lambda d: sg.fc_surrogate_test(rand(d, 66, 8, 3), surr_number=2, alpha=0.1, seeds=[3, 4],
                                                                 want_stats=True),
    # ---- utils ----
    "utils_envelope": lambda d: ut.envelope(nrand(44, 60), fcut=2.0),
    "utils_welch": lambda d: ut.welch(nrand(45, 3, 64), nperseg=8, nfft=8),
    "utils_spectrogram": lambda d: ut.spectrogram(nrand(45, 3, 64), nperseg=8, mode="phase"),
    "utils_csd": lambda d: ut.csd(nrand(45, 3, 64), nrand(46, 3, 64), nperseg=8),
    "utils_coherence": lambda d: ut.coherence(nrand(45, 64, 3), nrand(46, 64, 3), nperseg=8, axis=0),
    "utils_csd_matrix": lambda d: ut.csd_matrix(nrand(45, 64, 3), nperseg=8),
    "utils_coherence_matrix": lambda d: ut.coherence_matrix(nrand(45, 64, 3), nperseg=8),
    "utils_connectivity": lambda d: ut.connectivity(nrand(47, 60, 3).astype(np.float32), measures=("plv", "aec")),
    "utils_connectivity_no_band": lambda d: ut.connectivity(nrand(47, 60, 2, 3), freqs=None),
    "utils_fcd": lambda d: ut.fcd(nrand(48, 40, 3)),
    "utils_fcd_phase": lambda d: ut.fcd(nrand(48, 12, 2, 3), method="phase", trim=1),
    "utils_leida": lambda d: ut.leida(nrand(49, 60, 2, 3), 0.002, [8, 13], k=2, trim=2),
    "utils_leida_centroids": lambda d: ut.leida(nrand(49, 12, 3), 0.002, None, centroids=nrand(50, 2, 3)),
    "utils_kuramoto": lambda d: ut.kuramoto(nrand(51, 16, 3)),
    "utils_get_all_metrics": lambda d: ut.get_all_metrics(nweights(52, 8, 8), nweights(53, 8, 8)),
    "utils_host_helpers": lambda d: (ut.cohen_d(nrand(54, 9), nrand(55, 7)), ut.flat_FC(nrand(54, 4, 4)),
                                     ut.new_metric(nrand(54, 6), nrand(55, 6)), ut.sub_weight(nrand(54, 90, 90), 0.5),
                                     ut.cortex_mat(nrand(54, 90, 90)), ut.scale_mat(nrand(54, 90, 90), 0.2, 0.3)),
    # ---- graph_utils ----
    "graph_utils_distance_wei": lambda d: gu.distance_wei(nweights(56, 5, 5)),
    "graph_utils_efficiency_wei": lambda d: (gu.efficiency_wei(nweights(56, 5, 5)),
                                             gu.efficiency_wei(nweights(56, 2, 5, 5), local=True)),
    "graph_utils_clustering": lambda d: (gu.clustering_coef_wu(nweights(56, 5, 5)), gu.transitivity_wu(nweights(56, 5, 5)),
                                         gu.strengths_und(nweights(56, 2, 5, 5)), gu.degrees_und(nweights(56, 5, 5))),
    "graph_utils_betweenness": lambda d: (gu.betweenness_wei(nweights(56, 5, 5)),
                                          gu.betweenness_bin(nweights(56, 2, 5, 5) > 0.5)),
    "graph_utils_modules": lambda d: (gu.participation_coef(nweights(56, 5, 5), [3, 7, 3, 7, 7], degree="in"),
                                      gu.module_degree_zscore(nweights(56, 3, 5, 5), CI3, flag=2)),
    "graph_utils_community_louvain": lambda d: (gu.community_louvain(nweights(57, 5, 5), seed=1),
                                                gu.community_louvain(nweights(57, 2, 5, 5), gamma=0.8, ci=[1, 1, 2, 2, 3],
                                                                     B=nweights(58, 5, 5), seed=2)),
    "graph_utils_agreement": lambda d: gu.agreement(np.array([[1, 1, 2], [1, 2, 2], [3, 2, 2], [3, 3, 1]])),
    "graph_utils_get_agreement_matrix": lambda d: (gu.get_agreement_matrix(nweights(57, 5, 5), reps=2),
                                                   gu.get_agreement_matrix(nweights(57, 5, 5), reps=2, seeds=[4, 5])),
    "graph_utils_louvain_sign": lambda d: (ptn.modularity_louvain_und_sign(nsigned(67, 6, 6), seed=1),
                                           ptn.modularity_louvain_und_sign(nsigned(67, 2, 6, 6), gamma=0.8, qtype="gja",
                                                                           seed=2 ** 64 - 1)),
    "graph_utils_consensus_und": lambda d: (ptn.consensus_und(cliques("cpu").numpy(), 0.5, reps=2),
                                            ptn.consensus_und(cliques("cpu", 2).numpy(), 0.5, reps=3)),
    "graph_utils_null_models": lambda d: (nmn.randmio_und_signed(nsigned(69, 5, 5), 2, seed=1),
                                          nmn.null_model_und_sign(nsigned(69, 5, 5), bin_swaps=2, wei_freq=0.5, seed=2),
                                          nmn.participation_coef_norm(nsigned(69, 6, 6), CI6, BA_iters=2)),
    "graph_utils_probabilistic_thresholding": lambda d: (sgn.probabilistic_thresholding(nrand(68, 8, 3), surr_number=2),
                                                         sgn.probabilistic_thresholding(nrand(68, 2, 8, 3), 3, alpha=0.2)),
    "graph_utils_host_helpers": lambda d: (gu.get_uptri(nrand(59, 4, 4)), gu.matrix_recon(nrand(59, 6)),
                                           gu.thresholding(nweights(59, 6, 6), 0.5),
                                           gu.thresholding(nweights(59, 6, 6), 0.5, direct="directed"),
                                           gu.cuberoot(nrand(59, 5)), gu.invert(nweights(59, 4, 4)),
                                           gu.charpath(gu.invert(nweights(59, 4, 4) + np.eye(4)))),
}


@pytest.mark.parametrize("name", list(CASES))
def test_call_plan(name, cuda, recorder):
    CASES[name](cuda)
    assert recorder.calls == PLAN[name]


def test_every_case_has_a_plan():
    assert set(PLAN) == set(CASES)


def test_louvain_asymmetric_objective_warns(cuda, recorder):
    """The symmetrising warning fires after device work (one flag read back) and names the caller's file."""
    w = weights(cuda, 16, 3, 3)
    obj = rand(cuda, 17, 3, 3)
    with pytest.warns(UserWarning) as caught:
        ci, q = sc.graph_louvain(w, objective=obj)
    assert len(caught) == 1
    assert caught[0].category is UserWarning
    assert str(caught[0].message) == "graph_louvain: objective function matrix not symmetric, symmetrizing"
    assert caught[0].filename == __file__
    assert [c[0] for c in recorder.calls] == ["wc_graph_louvain"]
    sym = (obj + obj.t()) / 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ci2, q2 = sc.graph_louvain(w, objective=sym)
    assert torch.equal(ci, ci2) and torch.equal(q, q2)


def test_returned_views(cuda):
    """What the wrappers return as views stays a view: spectrogram's permuted buffer, fc_metrics' metrics[:, :K]."""
    _, _, sxx = sc.spectrogram(rand(cuda, 31, 64, 3), nperseg=8)
    assert tuple(sxx.shape) == (5, 3, 9) and not sxx.is_contiguous() and sxx.stride() == (3, 1, 15)
    _, met, _ = sc.fc_metrics(rand(cuda, 5, 8, 2 * 8), 2, 8)
    assert tuple(met.shape) == (2, 0, 4) and met._base is not None and tuple(met._base.shape) == (2, 1, 4)
    _, met, _ = sc.fc_metrics(rand(cuda, 5, 8, 2 * 8), 2, 8, empfc=nrand(6, 2, 8, 8))
    assert tuple(met.shape) == (2, 2, 4)


# What the proxy recorded at the commit before nremmodfc_amd/_args.py, on an MI355X.
PLAN = {'hilbert_phase_8192': [('wc_hilbert_phase', 2, 8192, 'p', 'p', 'p', 65536, 'p')],
 'hilbert_phase_8193': [('wc_hilbert_long_workspace_size', 2, 8193),
                        ('wc_hilbert_phase_long', 2, 8193, 'p', 'p', 'p', 2769152, 'p')],
 'hilbert_phase_long_explicit': [('wc_hilbert_long_workspace_size', 2, 100),
                                 ('wc_hilbert_phase_long', 2, 100, 'p', 'p', 'p', 4194304, 'p')],
 'hilbert_envelope_2047': [('wc_hilbert_envelope_workspace_size', 2, 2047, 0),
                           ('wc_hilbert_envelope', 2, 2047, 'p', 'p', 0, 'p', 16376, 'p')],
 'hilbert_envelope_2048': [('wc_hilbert_envelope_workspace_size', 2, 2048, 0),
                           ('wc_hilbert_envelope', 2, 2048, 'p', 'p', 0, 'p', 2670592, 'p')],
 'hilbert_envelope_2047_ws_below_min': [('wc_hilbert_envelope_workspace_size', 2, 2047, 0),
                                        ('wc_hilbert_envelope', 2, 2047, 'p', 'p', 0, 'p', 16376, 'p')],
 'hilbert_envelope_2048_explicit': [('wc_hilbert_envelope_workspace_size', 2, 2048, 0),
                                    ('wc_hilbert_envelope_workspace_size', 2, 2048, 0),
                                    ('wc_hilbert_envelope', 2, 2048, 'p', 'p', 0, 'p', 1626112, 'p')],
 'hilbert_envelope_method1': [('wc_hilbert_envelope_workspace_size', 2, 2048, 1),
                              ('wc_hilbert_envelope', 2, 2048, 'p', 'p', 1, 'p', 16384, 'p')],
 'hilbert_envelope_method2': [('wc_hilbert_envelope_workspace_size', 2, 100, 2),
                              ('wc_hilbert_envelope', 2, 100, 'p', 'p', 2, 'p', 2639616, 'p')],
 'fc_metrics_96_K0': [('wc_hilbert_phase', 192, 8, 'p', 'p', 'p', 64, 'p'),
                      ('wc_fc_metrics_workspace_size', 2, 96, 8, 0, 0),
                      ('wc_fc_metrics', 2, 96, 8, 'p', None, None, 0, 1.0, 'p', None, 'p', 'p', None, 0, 'p')],
 'fc_metrics_96_K1': [('wc_hilbert_phase', 192, 8, 'p', 'p', 'p', 64, 'p'),
                      ('wc_fc_metrics_workspace_size', 2, 96, 8, 1, 1),
                      ('wc_fc_metrics', 2, 96, 8, 'p', None, 'p', 1, 1.0, 'p', 'p', 'p', 'p', None, 0, 'p')],
 'fc_metrics_97_K0': [('wc_hilbert_phase', 194, 8, 'p', 'p', 'p', 64, 'p'),
                      ('wc_fc_metrics_workspace_size', 2, 97, 8, 0, 1),
                      ('wc_fc_metrics', 2, 97, 8, 'p', None, None, 0, 1.0, 'p', 'p', 'p', 'p', 'p', 3552, 'p')],
 'fc_metrics_97_K1_no_kuramoto': [('wc_fc_metrics_workspace_size', 2, 97, 8, 1, 0),
                                  ('wc_fc_metrics', 2, 97, 8, 'p', None, 'p', 1, 1.0, None, None, 'p', 'p', 'p',
                                   155344, 'p')],
 'fc_metrics_fc_in': [('wc_fc_metrics_workspace_size', 2, 8, 2, 2, 0),
                      ('wc_fc_metrics', 2, 8, 2, None, 'p', 'p', 2, 2.0, None, None, 'p', 'p', None, 0, 'p')],
 'hma_96': [('wc_hma', 2, 96, 'p', 'p', 'p', 'p', 'p', None, 'p', 'p')],
 'hma_96_clus_num': [('wc_hma', 2, 96, 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p')],
 'hma_2d': [('wc_hma', 1, 5, 'p', 'p', 'p', 'p', 'p', None, 'p', 'p')],
 'hma_97': [('wc_hma_modes', 2, 97, 'p', 'p', 'p', 'p', 'p', 'p', None, 'p', 'p')],
 'hma_97_clus_num': [('wc_hma_modes', 2, 97, 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p')],
 'hma_97_B65': [('wc_hma_modes', 64, 97, 'p', 'p', 'p', 'p', 'p', 'p', None, 'p', 'p'),
                ('wc_hma_modes', 1, 97, 'p', 'p', 'p', 'p', 'p', 'p', None, 'p', 'p')],
 'hma_97_B65_clus_num': [('wc_hma_modes', 64, 97, 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p'),
                         ('wc_hma_modes', 1, 97, 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p')],
 'graph_measures_dist': [('wc_graph_paths', 3, 5, 'p', 0, 1, 'p', None, None, None, 'p')],
 'graph_measures_degrees': [('wc_graph_clustering', 3, 5, 'p', None, None, None, 'p', 'p')],
 'graph_measures_all': [('wc_graph_paths', 3, 5, 'p', 0, 1, 'p', 'p', 'p', 'p', 'p'),
                        ('wc_graph_local_efficiency', 3, 5, 'p', 'p', 'p'),
                        ('wc_graph_clustering', 3, 5, 'p', 'p', 'p', 'p', 'p', 'p')],
 'graph_measures_paths_lengths': [('wc_graph_paths', 3, 5, 'p', 1, 0, None, None, 'p', 'p', 'p')],
 'graph_measures_N2_2d': [('wc_graph_paths', 1, 2, 'p', 0, 1, 'p', 'p', 'p', 'p', 'p'),
                          ('wc_graph_local_efficiency', 1, 2, 'p', 'p', 'p'),
                          ('wc_graph_clustering', 1, 2, 'p', 'p', 'p', 'p', 'p', 'p')],
 'graph_measures_N2_3d': [('wc_graph_paths', 1, 2, 'p', 0, 1, 'p', 'p', 'p', 'p', 'p'),
                          ('wc_graph_local_efficiency', 1, 2, 'p', 'p', 'p'),
                          ('wc_graph_clustering', 1, 2, 'p', 'p', 'p', 'p', 'p', 'p')],
 'graph_betweenness': [('wc_graph_betweenness', 3, 5, 'p', 0, 'p', 'p')],
 'graph_betweenness_2d_lengths': [('wc_graph_betweenness', 1, 5, 'p', 1, 'p', 'p')],
 'graph_module_measures_ci_1d': [('wc_graph_modules', 3, 5, 5, 'p', 'p', 0, 0, 1.0, 'p', 'p', 'p', 'p')],
 'graph_module_measures_ci_2d': [('wc_graph_modules', 3, 5, 2, 'p', 'p', 1, 3, 1.5, None, 'p', None, 'p')],
 'graph_module_measures_2d': [('wc_graph_modules', 1, 5, 5, 'p', 'p', 0, 0, 1.0, None, None, 'p', 'p')],
 'graph_louvain_seed_int': [('wc_graph_louvain', 1, 1, 3, 'p', 'p', None, 'p', 'p', 'p', None, 'p')],
 'graph_louvain_seeds_list_info': [('wc_graph_louvain', 2, 2, 3, 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p')],
 'graph_louvain_potts': [('wc_graph_louvain', 1, 1, 3, 'p', 'p', None, 'p', 'p', 'p', None, 'p')],
 'graph_louvain_objective_tensor': [('wc_graph_louvain', 1, 1, 3, 'p', 'p', None, 'p', 'p', 'p', None, 'p')],
 'graph_agreement': [('wc_graph_agreement', 2, 4, 5, 'p', 'p', 'p')],
 'graph_agreement_2d': [('wc_graph_agreement', 1, 4, 5, 'p', 'p', 'p')],
 'graph_consensus_matrix': [('wc_graph_louvain', 2, 2, 5, 'p', 'p', None, 'p', 'p', 'p', None, 'p'),
                            ('wc_graph_agreement', 2, 2, 5, 'p', 'p', 'p')],
 'graph_consensus_matrix_seeds': [('wc_graph_louvain', 1, 2, 5, 'p', 'p', None, 'p', 'p', 'p', None, 'p'),
                                  ('wc_graph_agreement', 1, 2, 5, 'p', 'p', 'p')],
 'fcd_corr': [('wc_fcd_workspace_size', 3, 3, 12, 4, 1), ('wc_fcd', 3, 3, 12, 'p', 4, 1, 'p', None, 'p', 864, 'p')],
 'fcd_corr_explicit_ws': [('wc_fcd_workspace_size', 3, 3, 12, 4, 2),
                          ('wc_fcd', 3, 3, 12, 'p', 4, 2, 'p', 'p', 'p', 65536, 'p')],
 'fcd_corr_2d': [('wc_fcd_workspace_size', 1, 3, 12, 4, 1),
                 ('wc_fcd', 1, 3, 12, 'p', 4, 1, 'p', 'p', 'p', 288, 'p')],
 'fcd_phase': [('wc_hilbert_phase', 9, 12, 'p', 'p', 'p', 96, 'p'), ('wc_fcd_phase', 3, 3, 10, 'p', 'p', 'p')],
 'fcd_phase_2d': [('wc_hilbert_phase', 3, 12, 'p', 'p', 'p', 96, 'p'), ('wc_fcd_phase', 1, 3, 12, 'p', 'p', 'p')],
 'fcd_from_phasors': [('wc_fcd_phase', 2, 3, 6, 'p', 'p', 'p')],
 'fcd_from_phasors_3d': [('wc_fcd_phase', 1, 3, 6, 'p', 'p', 'p')],
 'fcd_ks': [('wc_fcd_workspace_size', 3, 3, 12, 4, 1), ('wc_fcd', 3, 3, 12, 'p', 4, 1, 'p', None, 'p', 864, 'p')],
 'leida': [('wc_hilbert_phase', 6, 12, 'p', 'p', 'p', 96, 'p'), ('wc_leida_eigvec', 20, 3, 'p', 'p', 'p', 'p')],
 'leida_2d': [('wc_hilbert_phase', 3, 12, 'p', 'p', 'p', 96, 'p'), ('wc_leida_eigvec', 12, 3, 'p', 'p', 'p', 'p')],
 'leida_from_phasors': [('wc_leida_eigvec', 12, 3, 'p', 'p', 'p', 'p')],
 'leida_from_phasors_offset': [('wc_leida_eigvec', 6, 3, 'p', 'p', 'p', 'p')],
 'kmeans_assign': [('wc_kmeans_assign', 8, 3, 2, 'p', 'p', 0, 'p', 'p', 'p')],
 'kmeans_update': [('wc_kmeans_assign', 8, 2, 2, 'p', 'p', 1, 'p', 'p', 'p'),
                   ('wc_kmeans_workspace_size', 8, 2, 2, 1),
                   ('wc_kmeans_update', 8, 2, 2, 'p', 'p', 'p', 1, 'p', 'p', 'p', 112, 'p'),
                   ('wc_kmeans_update', 8, 2, 2, 'p', 'p', 'p', 0, 'p', 'p', 'p', 65536, 'p')],
 'kmeans_k': [('wc_kmeans_assign', 8, 2, 2, 'p', 'p', 1, 'p', 'p', 'p'), ('wc_kmeans_workspace_size', 8, 2, 2, 1),
              ('wc_kmeans_update', 8, 2, 2, 'p', 'p', 'p', 1, 'p', 'p', 'p', 112, 'p'),
              ('wc_kmeans_assign', 8, 2, 2, 'p', 'p', 1, 'p', 'p', 'p')],
 'kmeans_init': [('wc_kmeans_assign', 8, 2, 2, 'p', 'p', 0, 'p', 'p', 'p'),
                 ('wc_kmeans_workspace_size', 8, 2, 2, 0),
                 ('wc_kmeans_update', 8, 2, 2, 'p', 'p', 'p', 0, 'p', 'p', 'p', 48, 'p'),
                 ('wc_kmeans_assign', 8, 2, 2, 'p', 'p', 0, 'p', 'p', 'p'),
                 ('wc_kmeans_workspace_size', 8, 2, 2, 0),
                 ('wc_kmeans_update', 8, 2, 2, 'p', 'p', 'p', 0, 'p', 'p', 'p', 48, 'p'),
                 ('wc_kmeans_assign', 8, 2, 2, 'p', 'p', 0, 'p', 'p', 'p')],
 'state_stats': [('wc_state_stats', 2, 20, 3, 'p', 'p', 'p', 'p', 'p')],
 'state_stats_1d': [('wc_state_stats', 1, 20, 3, 'p', 'p', 'p', 'p', 'p')],
 'leida_states': [('wc_kmeans_assign', 12, 3, 2, 'p', 'p', 1, 'p', 'p', 'p'),
                  ('wc_state_stats', 2, 6, 2, 'p', 'p', 'p', 'p', 'p')],
 'leida_states_2d': [('wc_kmeans_assign', 6, 3, 2, 'p', 'p', 0, 'p', 'p', 'p'),
                     ('wc_state_stats', 1, 6, 2, 'p', 'p', 'p', 'p', 'p')],
 'state_kl': [],
 'welch': [('wc_welch_psd_workspace_size', 3, 64, 8, 4),
           ('wc_welch_psd', 3, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 'p', 'p', 133312, 'p')],
 'welch_3d_explicit_ws': [('wc_welch_psd_workspace_size', 3, 64, 8, 2),
                          ('wc_welch_psd', 3, 64, 'p', 8, 2, 'p', 0, 0.08163265306122448, 'p', 'p', 1048576, 'p')],
 'csd_matrix': [('wc_csd_workspace_size', 3, 64, 8, 4),
                ('wc_csd', 3, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 0, 'p', 'p', 136432, 'p')],
 'csd_pairs': [('wc_csd_workspace_size', 6, 64, 8, 4),
               ('wc_csd', 6, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 2, 'p', 'p', 1048576, 'p')],
 'coherence_matrix': [('wc_csd_workspace_size', 3, 64, 8, 4),
                      ('wc_csd', 3, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 1, 'p', 'p', 136432, 'p')],
 'coherence_pairs': [('wc_csd_workspace_size', 6, 64, 8, 4),
                     ('wc_csd', 6, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 3, 'p', 'p', 140512, 'p')],
 'spectrogram': [('wc_spectrogram_workspace_size', 8),
                 ('wc_spectrogram', 3, 64, 'p', 8, 1, 'p', 1, 0.14285714285714285, 0, 'p', 'p', 132352, 'p')],
 'spectrogram_3d_complex': [('wc_spectrogram_workspace_size', 8),
                            ('wc_spectrogram', 3, 64, 'p', 8, 4, 'p', 1, 0.14285714285714285, 1, 'p', 'p', 132352,
                             'p')],
 'phase_connectivity_from_all': [('wc_phase_conn_workspace_size', 2, 3, 16, 15),
                                 ('wc_phase_conn', 2, 3, 16, 'p', 'p', 15, 'p', 'p', 131168, 'p'),
                                 ('wc_corrcoef_workspace_size', 2, 3, 16),
                                 ('wc_corrcoef', 2, 3, 16, 'p', 'p', 'p', 248, 'p')],
 'phase_connectivity_from_plv_3d': [('wc_phase_conn_workspace_size', 1, 3, 16, 1),
                                    ('wc_phase_conn', 1, 3, 16, 'p', None, 1, 'p', 'p', 65536, 'p')],
 'phase_connectivity_from_aec_N1': [],
 'phase_connectivity_from_aec_97': [('wc_corrcoef_workspace_size', 1, 48, 16),
                                    ('wc_corrcoef', 1, 48, 16, 'p', 'p', 'p', 19208, 'p'),
                                    ('wc_corrcoef_workspace_size', 1, 96, 16),
                                    ('wc_corrcoef', 1, 96, 16, 'p', 'p', 'p', 75272, 'p'),
                                    ('wc_corrcoef_workspace_size', 1, 49, 16),
                                    ('wc_corrcoef', 1, 49, 16, 'p', 'p', 'p', 20000, 'p'),
                                    ('wc_corrcoef_workspace_size', 1, 48, 16),
                                    ('wc_corrcoef', 1, 48, 16, 'p', 'p', 'p', 19208, 'p'),
                                    ('wc_corrcoef_workspace_size', 1, 49, 16),
                                    ('wc_corrcoef', 1, 49, 16, 'p', 'p', 'p', 20000, 'p')],
 'phase_connectivity': [('wc_hilbert_phase', 6, 16, 'p', 'p', 'p', 128, 'p'),
                        ('wc_hilbert_envelope_workspace_size', 6, 16, 0),
                        ('wc_hilbert_envelope', 6, 16, 'p', 'p', 0, 'p', 128, 'p'),
                        ('wc_phase_conn_workspace_size', 2, 3, 16, 15),
                        ('wc_phase_conn', 2, 3, 16, 'p', 'p', 15, 'p', 'p', 131168, 'p'),
                        ('wc_corrcoef_workspace_size', 2, 3, 16),
                        ('wc_corrcoef', 2, 3, 16, 'p', 'p', 'p', 248, 'p')],
 'phase_connectivity_pli': [('wc_hilbert_phase', 3, 16, 'p', 'p', 'p', 128, 'p'),
                            ('wc_phase_conn_workspace_size', 1, 3, 16, 3),
                            ('wc_phase_conn', 1, 3, 16, 'p', None, 3, 'p', 'p', 24576, 'p')],
 'filtfilt': [('wc_filtfilt', 1, [0.2, 0.3], [1.0, -0.5], [0.8], 30, 4, 'p', 'p', 'p')],
 'envelope': [('wc_filtfilt', 6,
               [2.876655637767032e-05, 0.0, -8.629966913301096e-05, 0.0, 8.629966913301096e-05, 0.0,
                -2.876655637767032e-05],
               [1.0, -5.80109048161183, 14.068373306109635, -18.25583446088042, 13.369172551840377,
                -5.2388321125792014, 0.8582152898598835],
               [-2.8766556374879946e-05, -2.8766556391067163e-05, 5.753311278119981e-05, 5.753311273025923e-05,
                -2.8766556365446774e-05, -2.876655638006506e-05],
               60, 2, 'p', 'p', 'p'),
              ('wc_hilbert_envelope_workspace_size', 2, 60, 0),
              ('wc_hilbert_envelope', 2, 60, 'p', 'p', 0, 'p', 480, 'p')],
 'envelope_fcut': [('wc_filtfilt', 6,
                    [2.876655637767032e-05, 0.0, -8.629966913301096e-05, 0.0, 8.629966913301096e-05, 0.0,
                     -2.876655637767032e-05],
                    [1.0, -5.80109048161183, 14.068373306109635, -18.25583446088042, 13.369172551840377,
                     -5.2388321125792014, 0.8582152898598835],
                    [-2.8766556374879946e-05, -2.8766556391067163e-05, 5.753311278119981e-05, 5.753311273025923e-05,
                     -2.8766556365446774e-05, -2.876655638006506e-05],
                    60, 2, 'p', 'p', 'p'),
                   ('wc_hilbert_envelope_workspace_size', 2, 60, 0),
                   ('wc_hilbert_envelope', 2, 60, 'p', 'p', 0, 'p', 480, 'p'),
                   ('wc_filtfilt', 3,
                    [1.925103198861916e-06, 5.775309596585749e-06, 5.775309596585749e-06, 1.925103198861916e-06],
                    [1.0, -2.939165718919677, 2.879865703434369, -0.9406845836891014],
                    [0.9999980749238196, -1.9391734193848662, 0.9406865088177162], 60, 2, 'p', 'p', 'p')],
 'kuramoto': [('wc_hilbert_phase', 6, 16, 'p', 'p', 'p', 128, 'p'), ('wc_kuramoto', 2, 3, 16, 'p', 'p', 'p')],
 'corrcoef': [('wc_corrcoef_workspace_size', 2, 3, 16), ('wc_corrcoef', 2, 3, 16, 'p', 'p', 'p', 248, 'p')],
 'sim_bold': [('wc_bold_blocks',
               {'dt': 0.04,
                'neq': 2000,
                'n_total': 2016,
                'dec': 1000,
                'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                       0.00012544743181345855]}),
              ('wc_bold_state_doubles',
               {'dt': 0.04,
                'neq': 2000,
                'n_total': 2016,
                'dec': 1000,
                'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                       0.00012544743181345855]},
               2),
              ('wc_bold_init',
               {'dt': 0.04,
                'neq': 2000,
                'n_total': 2016,
                'dec': 1000,
                'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                       0.00012544743181345855]},
               2, 'p', 'p'),
              ('wc_bold_chunk',
               {'dt': 0.04,
                'neq': 2000,
                'n_total': 2016,
                'dec': 1000,
                'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                       0.00012544743181345855]},
               2, 'p', 1, 0, 0, 2016, 'p', None, 0, 'p'),
              ('wc_bold_finish',
               {'dt': 0.04,
                'neq': 2000,
                'n_total': 2016,
                'dec': 1000,
                'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                       0.00012544743181345855]},
               2, 'p', 'p', 'p')],
 'welch_peak': [('wc_welch_bins',), ('wc_welch_workspace_size',), ('wc_welch_prepare', 'p', 127960, 'p'),
                ('wc_welch_accumulate', 1, 1, 'p', 1, 8000, 8000, 1, 0, 1, 'p', 'p', 'p'),
                ('wc_welch_accumulate', 1, 1, 'p', 1, 8000, 8000, 1, 2000, 1, 'p', 'p', 'p'),
                ('wc_welch_accumulate', 1, 1, 'p', 1, 8000, 8000, 1, 4000, 1, 'p', 'p', 'p'),
                ('wc_welch_peak', 1, 1, 3, 500.0, 'p', 'p', 'p', 'p')],
 'bold_stream': [('wc_bold_blocks',
                  {'dt': 0.04,
                   'neq': 2000,
                   'n_total': 2016,
                   'dec': 1000,
                   'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                   'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                   'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                          0.00012544743181345855]}),
                 ('wc_bold_state_doubles',
                  {'dt': 0.04,
                   'neq': 2000,
                   'n_total': 2016,
                   'dec': 1000,
                   'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                   'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                   'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                          0.00012544743181345855]},
                  2),
                 ('wc_bold_init',
                  {'dt': 0.04,
                   'neq': 2000,
                   'n_total': 2016,
                   'dec': 1000,
                   'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                   'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                   'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                          0.00012544743181345855]},
                  2, 'p', 'p'),
                 ('wc_bold_chunk',
                  {'dt': 0.04,
                   'neq': 2000,
                   'n_total': 2016,
                   'dec': 1000,
                   'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                   'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                   'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                          0.00012544743181345855]},
                  2, 'p', 0, 0, 0, 1000, 'p', 'p', 4000, 'p'),
                 ('wc_bold_chunk',
                  {'dt': 0.04,
                   'neq': 2000,
                   'n_total': 2016,
                   'dec': 1000,
                   'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                   'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                   'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                          0.00012544743181345855]},
                  2, 'p', 1, 0, 1000, 1016, 'p', None, 0, 'p'),
                 ('wc_bold_finish',
                  {'dt': 0.04,
                   'neq': 2000,
                   'n_total': 2016,
                   'dec': 1000,
                   'b': [0.00012544743505202416, 0.0, -0.0002508948701040483, 0.0, 0.00012544743505202416],
                   'a': [1.0, -3.9609509668036016, 5.883482227394972, -3.8841091195101143, 0.9615778628317615],
                   'zi': [-0.00012544743168405392, -0.000125447445024419, 0.00012544744489502245,
                          0.00012544743181345855]},
                  2, 'p', 'p', 'p')],
 'welch_accumulator': [('wc_welch_bins',), ('wc_welch_workspace_size',), ('wc_welch_prepare', 'p', 127960, 'p'),
                       ('wc_welch_accumulate', 1, 1, 'p', 0, 4000, 1000, 4, 0, 1, 'p', 'p', 'p'),
                       ('wc_welch_accumulate', 1, 1, 'p', 0, 4000, 1000, 4, 2000, 1, 'p', 'p', 'p'),
                       ('wc_welch_peak', 1, 1, 2, 500.0, 'p', 'p', 'p', 'p')],
 'utils_envelope': [('wc_filtfilt', 6,
                     [2.876655637767032e-05, 0.0, -8.629966913301096e-05, 0.0, 8.629966913301096e-05, 0.0,
                      -2.876655637767032e-05],
                     [1.0, -5.80109048161183, 14.068373306109635, -18.25583446088042, 13.369172551840377,
                      -5.2388321125792014, 0.8582152898598835],
                     [-2.8766556374879946e-05, -2.8766556391067163e-05, 5.753311278119981e-05,
                      5.753311273025923e-05, -2.8766556365446774e-05, -2.876655638006506e-05],
                     60, 1, 'p', 'p', 'p'),
                    ('wc_hilbert_envelope_workspace_size', 1, 60, 0),
                    ('wc_hilbert_envelope', 1, 60, 'p', 'p', 0, 'p', 480, 'p'),
                    ('wc_filtfilt', 3,
                     [1.925103198861916e-06, 5.775309596585749e-06, 5.775309596585749e-06, 1.925103198861916e-06],
                     [1.0, -2.939165718919677, 2.879865703434369, -0.9406845836891014],
                     [0.9999980749238196, -1.9391734193848662, 0.9406865088177162], 60, 1, 'p', 'p', 'p')],
 'utils_welch': [('wc_welch_psd_workspace_size', 3, 64, 8, 4),
                 ('wc_welch_psd', 3, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 'p', 'p', 133312, 'p')],
 'utils_spectrogram': [('wc_spectrogram_workspace_size', 8),
                       ('wc_spectrogram', 3, 64, 'p', 8, 1, 'p', 1, 0.14285714285714285, 3, 'p', 'p', 132352, 'p')],
 'utils_csd': [('wc_csd_workspace_size', 6, 64, 8, 4),
               ('wc_csd', 6, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 2, 'p', 'p', 140512, 'p')],
 'utils_coherence': [('wc_csd_workspace_size', 6, 64, 8, 4),
                     ('wc_csd', 6, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 3, 'p', 'p', 140512, 'p')],
 'utils_csd_matrix': [('wc_csd_workspace_size', 3, 64, 8, 4),
                      ('wc_csd', 3, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 0, 'p', 'p', 136432, 'p')],
 'utils_coherence_matrix': [('wc_csd_workspace_size', 3, 64, 8, 4),
                            ('wc_csd', 3, 64, 'p', 8, 4, 'p', 1, 0.3333333333333333, 1, 'p', 'p', 136432, 'p')],
 'utils_connectivity': [('wc_filtfilt', 6,
                         [2.876655637767032e-05, 0.0, -8.629966913301096e-05, 0.0, 8.629966913301096e-05, 0.0,
                          -2.876655637767032e-05],
                         [1.0, -5.80109048161183, 14.068373306109635, -18.25583446088042, 13.369172551840377,
                          -5.2388321125792014, 0.8582152898598835],
                         [-2.8766556374879946e-05, -2.8766556391067163e-05, 5.753311278119981e-05,
                          5.753311273025923e-05, -2.8766556365446774e-05, -2.876655638006506e-05],
                         60, 3, 'p', 'p', 'p'),
                        ('wc_hilbert_phase', 3, 60, 'p', 'p', 'p', 480, 'p'),
                        ('wc_hilbert_envelope_workspace_size', 3, 60, 0),
                        ('wc_hilbert_envelope', 3, 60, 'p', 'p', 0, 'p', 480, 'p'),
                        ('wc_phase_conn_workspace_size', 1, 3, 60, 1),
                        ('wc_phase_conn', 1, 3, 60, 'p', None, 1, 'p', 'p', 24576, 'p'),
                        ('wc_corrcoef_workspace_size', 1, 3, 60),
                        ('wc_corrcoef', 1, 3, 60, 'p', 'p', 'p', 128, 'p')],
 'utils_connectivity_no_band': [('wc_hilbert_phase', 6, 60, 'p', 'p', 'p', 480, 'p'),
                                ('wc_hilbert_envelope_workspace_size', 6, 60, 0),
                                ('wc_hilbert_envelope', 6, 60, 'p', 'p', 0, 'p', 480, 'p'),
                                ('wc_phase_conn_workspace_size', 2, 3, 60, 15),
                                ('wc_phase_conn', 2, 3, 60, 'p', 'p', 15, 'p', 'p', 131168, 'p'),
                                ('wc_corrcoef_workspace_size', 2, 3, 60),
                                ('wc_corrcoef', 2, 3, 60, 'p', 'p', 'p', 248, 'p')],
 'utils_fcd': [('wc_fcd_workspace_size', 1, 3, 40, 30, 1),
               ('wc_fcd', 1, 3, 40, 'p', 30, 1, 'p', None, 'p', 352, 'p')],
 'utils_fcd_phase': [('wc_hilbert_phase', 6, 12, 'p', 'p', 'p', 96, 'p'),
                     ('wc_fcd_phase', 2, 3, 10, 'p', 'p', 'p')],
 'utils_leida': [('wc_filtfilt', 6,
                  [2.876655637767032e-05, 0.0, -8.629966913301096e-05, 0.0, 8.629966913301096e-05, 0.0,
                   -2.876655637767032e-05],
                  [1.0, -5.80109048161183, 14.068373306109635, -18.25583446088042, 13.369172551840377,
                   -5.2388321125792014, 0.8582152898598835],
                  [-2.8766556374879946e-05, -2.8766556391067163e-05, 5.753311278119981e-05, 5.753311273025923e-05,
                   -2.8766556365446774e-05, -2.876655638006506e-05],
                  60, 6, 'p', 'p', 'p'),
                 ('wc_hilbert_phase', 6, 60, 'p', 'p', 'p', 480, 'p'),
                 ('wc_leida_eigvec', 112, 3, 'p', 'p', 'p', 'p'),
                 ('wc_kmeans_assign', 112, 3, 2, 'p', 'p', 1, 'p', 'p', 'p'),
                 ('wc_kmeans_workspace_size', 112, 3, 2, 1),
                 ('wc_kmeans_update', 112, 3, 2, 'p', 'p', 'p', 1, 'p', 'p', 'p', 960, 'p'),
                 ('wc_kmeans_assign', 112, 3, 2, 'p', 'p', 1, 'p', 'p', 'p'),
                 ('wc_kmeans_assign', 112, 3, 2, 'p', 'p', 1, 'p', 'p', 'p'),
                 ('wc_state_stats', 2, 56, 2, 'p', 'p', 'p', 'p', 'p')],
 'utils_leida_centroids': [('wc_hilbert_phase', 3, 12, 'p', 'p', 'p', 96, 'p'),
                           ('wc_leida_eigvec', 12, 3, 'p', 'p', 'p', 'p'),
                           ('wc_kmeans_assign', 12, 3, 2, 'p', 'p', 1, 'p', 'p', 'p'),
                           ('wc_state_stats', 1, 12, 2, 'p', 'p', 'p', 'p', 'p')],
 'utils_kuramoto': [('wc_hilbert_phase', 3, 16, 'p', 'p', 'p', 128, 'p'), ('wc_kuramoto', 1, 3, 16, 'p', 'p', 'p')],
 'utils_get_all_metrics': [('wc_fc_metrics_workspace_size', 1, 8, 2, 1, 0),
                           ('wc_fc_metrics', 1, 8, 2, None, 'p', 'p', 1, 1.0, None, None, 'p', 'p', None, 0, 'p')],
 'utils_host_helpers': [],
 'graph_utils_distance_wei': [('wc_graph_paths', 1, 5, 'p', 1, 1, 'p', 'p', None, None, 'p')],
 'graph_utils_efficiency_wei': [('wc_graph_paths', 1, 5, 'p', 0, 1, None, None, 'p', None, 'p'),
                                ('wc_graph_local_efficiency', 2, 5, 'p', 'p', 'p')],
 'graph_utils_clustering': [('wc_graph_clustering', 1, 5, 'p', 'p', None, None, None, 'p'),
                            ('wc_graph_clustering', 1, 5, 'p', None, 'p', None, None, 'p'),
                            ('wc_graph_clustering', 2, 5, 'p', None, None, 'p', None, 'p'),
                            ('wc_graph_clustering', 1, 5, 'p', None, None, None, 'p', 'p')],
 'graph_utils_betweenness': [('wc_graph_betweenness', 1, 5, 'p', 1, 'p', 'p'),
                             ('wc_graph_betweenness', 2, 5, 'p', 1, 'p', 'p')],
 'graph_utils_modules': [('wc_graph_modules', 1, 5, 2, 'p', 'p', 1, 0, 1.0, 'p', None, None, 'p'),
                         ('wc_graph_modules', 3, 5, 2, 'p', 'p', 0, 2, 1.0, None, 'p', None, 'p')],
 'graph_utils_community_louvain': [('wc_graph_louvain', 1, 1, 5, 'p', 'p', None, 'p', 'p', 'p', None, 'p'),
                                   ('wc_graph_louvain', 2, 1, 5, 'p', 'p', 'p', 'p', 'p', 'p', None, 'p')],
 'graph_utils_agreement': [('wc_graph_agreement', 1, 3, 4, 'p', 'p', 'p')],
 'graph_utils_get_agreement_matrix': [('wc_graph_louvain', 1, 2, 5, 'p', 'p', None, 'p', 'p', 'p', None, 'p'),
                                      ('wc_graph_agreement', 1, 2, 5, 'p', 'p', 'p'),
                                      ('wc_graph_louvain', 1, 2, 5, 'p', 'p', None, 'p', 'p', 'p', None, 'p'),
                                      ('wc_graph_agreement', 1, 2, 5, 'p', 'p', 'p')],
 'graph_utils_host_helpers': [],
 # recorded at the commit before the seeded wrappers moved onto _args.py's seeded-run helpers, on an MI355X
 'louvain_sign_seeds_u64_info': [('wc_graph_louvain_sign', 2, 2, 6, 'p', 1.0, 0, 'p', 'p', 'p', 'p', 'p', 2304, 'p')],
 'louvain_sign_seed_int_2d': [('wc_graph_louvain_sign', 1, 1, 6, 'p', 0.9, 4, 'p', 'p', 'p', None, 'p', 576, 'p')],
 'louvain_sign_one_slot': [('wc_graph_louvain_sign', 2, 2, 6, 'p', 1.0, 2, 'p', 'p', 'p', None, 'p', 576, 'p')],
 'graph_consensus': [('wc_graph_louvain_sign', 1, 2, 6, 'p', 1.0, 0, 'p', 'p', 'p', None, 'p', 1152, 'p'),
                     ('wc_graph_agreement', 1, 2, 6, 'p', 'p', 'p')],
 'graph_consensus_batch_seeds': [('wc_graph_louvain_sign', 2, 2, 6, 'p', 1.0, 0, 'p', 'p', 'p', None, 'p', 2304, 'p'),
                                 ('wc_graph_agreement', 2, 2, 6, 'p', 'p', 'p')],
 'graph_rewire_N4': [('wc_graph_rewire', 1, 1, 4, 'p', 5, 'p', 'p', None, 'p', 48, 'p')],
 'graph_rewire_N5_info_one_slot': [('wc_graph_rewire', 2, 2, 5, 'p', 3, 'p', 'p', 'p', 'p', 80, 'p')],
 'graph_null_model_N4': [('wc_graph_null_model', 1, 1, 4, 'p', 5, 10, 1, 'p', 'p', None, None, 'p', 48, 'p')],
 'graph_null_model_N5_stats_one_slot': [('wc_graph_null_model', 2, 2, 5, 'p', 2, 2, 0, 'p', 'p', 'p', 'p', 'p', 80,
                                         'p')],
 'graph_null_model_sorted_once': [('wc_graph_null_model', 1, 1, 5, 'p', 5, 0, 1, 'p', 'p', 'p', 'p', 'p', 80, 'p')],
 'participation_norm_chunks': [('wc_graph_null_model', 2, 1, 6, 'p', 5, 10, 1, 'p', 'p', 'p', 'p', 'p', 240, 'p'),
                               ('wc_graph_null_model', 2, 1, 6, 'p', 5, 10, 1, 'p', 'p', 'p', 'p', 'p', 240, 'p'),
                               ('wc_graph_null_model', 2, 1, 6, 'p', 5, 10, 1, 'p', 'p', 'p', 'p', 'p', 240, 'p')],
 'participation_norm_2d_seeds': [('wc_graph_null_model', 1, 2, 6, 'p', 1, 1, 0, 'p', 'p', 'p', 'p', 'p', 240, 'p')],
 'surrogate_fc': [('wc_spectrogram_workspace_size', 4),
                  ('wc_spectrogram', 2, 4, 'p', 4, 0, 'p', 1, 1.0, 1, 'p', 'p', 132352, 'p'),
                  ('wc_surrogate_fc', 1, 2, 4, 2, 'p', 'p', 'p', 'p')],
 'surrogate_fc_3d_u64': [('wc_spectrogram_workspace_size', 4),
                         ('wc_spectrogram', 4, 4, 'p', 4, 0, 'p', 1, 1.0, 1, 'p', 'p', 132352, 'p'),
                         ('wc_surrogate_fc', 2, 2, 4, 2, 'p', 'p', 'p', 'p')],
 'fc_surrogate_test_chunks': [('wc_spectrogram_workspace_size', 8),
                              ('wc_spectrogram', 3, 8, 'p', 8, 0, 'p', 1, 1.0, 1, 'p', 'p', 132352, 'p'),
                              ('wc_surrogate_fc', 1, 3, 8, 2, 'p', 'p', 'p', 'p'),
                              ('wc_corrcoef_workspace_size', 1, 3, 8),
                              ('wc_corrcoef', 1, 3, 8, 'p', 'p', 'p', 128, 'p'),
                              ('wc_surrogate_test', 1, 3, 2, 'p', 'p', 0.05, 'p', 'p', None, None, None, 'p'),
                              ('wc_spectrogram_workspace_size', 8),
                              ('wc_spectrogram', 3, 8, 'p', 8, 0, 'p', 1, 1.0, 1, 'p', 'p', 132352, 'p'),
                              ('wc_surrogate_fc', 1, 3, 8, 2, 'p', 'p', 'p', 'p'),
                              ('wc_corrcoef_workspace_size', 1, 3, 8),
                              ('wc_corrcoef', 1, 3, 8, 'p', 'p', 'p', 128, 'p'),
                              ('wc_surrogate_test', 1, 3, 2, 'p', 'p', 0.05, 'p', 'p', None, None, None, 'p'),
                              ('wc_spectrogram_workspace_size', 8),
                              ('wc_spectrogram', 3, 8, 'p', 8, 0, 'p', 1, 1.0, 1, 'p', 'p', 132352, 'p'),
                              ('wc_surrogate_fc', 1, 3, 8, 2, 'p', 'p', 'p', 'p'),
                              ('wc_corrcoef_workspace_size', 1, 3, 8),
                              ('wc_corrcoef', 1, 3, 8, 'p', 'p', 'p', 128, 'p'),
                              ('wc_surrogate_test', 1, 3, 2, 'p', 'p', 0.05, 'p', 'p', None, None, None, 'p')],
 'fc_surrogate_test_2d_stats': [('wc_spectrogram_workspace_size', 8),
                                ('wc_spectrogram', 3, 8, 'p', 8, 0, 'p', 1, 1.0, 1, 'p', 'p', 132352, 'p'),
                                ('wc_surrogate_fc', 1, 3, 8, 2, 'p', 'p', 'p', 'p'),
                                ('wc_corrcoef_workspace_size', 1, 3, 8),
                                ('wc_corrcoef', 1, 3, 8, 'p', 'p', 'p', 128, 'p'),
                                ('wc_surrogate_test', 1, 3, 2, 'p', 'p', 0.1, 'p', 'p', 'p', 'p', 'p', 'p')],
 'graph_utils_louvain_sign': [('wc_graph_louvain_sign', 1, 1, 6, 'p', 1.0, 0, 'p', 'p', 'p', None, 'p', 576, 'p'),
                              ('wc_graph_louvain_sign', 2, 1, 6, 'p', 0.8, 3, 'p', 'p', 'p', None, 'p', 1152, 'p')],
 'graph_utils_consensus_und': [('wc_graph_louvain_sign', 1, 2, 6, 'p', 1.0, 0, 'p', 'p', 'p', None, 'p', 1152, 'p'),
                               ('wc_graph_agreement', 1, 2, 6, 'p', 'p', 'p'),
                               ('wc_graph_louvain_sign', 2, 3, 6, 'p', 1.0, 0, 'p', 'p', 'p', None, 'p', 3456, 'p'),
                               ('wc_graph_agreement', 2, 3, 6, 'p', 'p', 'p')],
 'graph_utils_null_models': [('wc_graph_rewire', 1, 1, 5, 'p', 2, 'p', 'p', 'p', 'p', 80, 'p'),
                             ('wc_graph_null_model', 1, 1, 5, 'p', 2, 2, 0, 'p', 'p', 'p', 'p', 'p', 80, 'p'),
                             ('wc_graph_null_model', 1, 2, 6, 'p', 5, 10, 0, 'p', 'p', 'p', 'p', 'p', 240, 'p')],
 'graph_utils_probabilistic_thresholding': [('wc_spectrogram_workspace_size', 8),
                                            ('wc_spectrogram', 3, 8, 'p', 8, 0, 'p', 1, 1.0, 1, 'p', 'p', 132352, 'p'),
                                            ('wc_surrogate_fc', 1, 3, 8, 2, 'p', 'p', 'p', 'p'),
                                            ('wc_corrcoef_workspace_size', 1, 3, 8),
                                            ('wc_corrcoef', 1, 3, 8, 'p', 'p', 'p', 128, 'p'),
                                            ('wc_surrogate_test', 1, 3, 2, 'p', 'p', 0.05, 'p', 'p', None, None, None,
                                             'p'),
                                            ('wc_spectrogram_workspace_size', 8),
                                            ('wc_spectrogram', 6, 8, 'p', 8, 0, 'p', 1, 1.0, 1, 'p', 'p', 132352, 'p'),
                                            ('wc_surrogate_fc', 2, 3, 8, 3, 'p', 'p', 'p', 'p'),
                                            ('wc_corrcoef_workspace_size', 2, 3, 8),
                                            ('wc_corrcoef', 2, 3, 8, 'p', 'p', 'p', 248, 'p'),
                                            ('wc_surrogate_test', 2, 3, 3, 'p', 'p', 0.2, 'p', 'p', None, None, None,
                                             'p')]}
