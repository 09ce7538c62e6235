"""gwamd — MI355X-native node2vec walk generation and TopSim SimRank.

Host-side mirror of the reference interfaces over the libgraphwalk C ABI
(include/graphwalk.h):

* `gwamd.node2vec`  — node2vec/src/node2vec.py (Graph, alias_setup, alias_draw)
* `gwamd.embed`     — learn_embeddings (node2vec/src/main.py:92-101): skip-gram /
                      negative-sampling training on the device-resident walks,
                      save_word2vec_format
* `gwamd.deepsim`   — DeepSim/src/DeepSim.py (main, save_embeddings): the SimRank-guided
                      net trained on the device-resident walks and SimRank rows;
                      `python -m gwamd.deepsim` takes DeepSim/src/main.py's flags
* `gwamd.classify`  — classify.scoring (node2vec/src/classify.py): one-vs-rest logistic
                      regression on the device-resident embedding, top-k prediction,
                      micro- / macro-F1; `python -m gwamd.classify --emb X --groups G`
* `gwamd.neighbors` — KeyedVectors.most_similar (DeepSim/src/main.py:287): all-pairs top-k
                      cosine / dot neighbours of the device-resident embedding, in gw_topsim's
                      row layout; label_agreement (preprocess_simrank);
                      `python -m gwamd.neighbors --emb X --output X.nn`
* `gwamd.eigenmaps` — IsoMap_LE/simRank.py learn_embeddings (Laplacian eigenmaps of SimRank top-k
                      rows, or of a graph's adjacency), sparse and symmetrised, in fp64;
                      `python -m gwamd.eigenmaps --simrank X.sim.txt --output X.emb`
* `gwamd.pointgraph` — IsoMap_LE/LE.py knn and heat-kernel weights: the k Euclidean nearest
                      neighbours of device-resident points, in gw_topsim's row layout;
                      eigenmaps.eigenmaps_of_points / laplaEigen chain it into the solver
                      (`python -m gwamd.eigenmaps --points X.npy --knn 10 --heat 15`)
* `gwamd.topsim`    — DeepSim/TopSimAll structures.Graph, TopSim_singleSample,
                      TopSim_Enumerate, SingleRandomWalk, SimRank (naive),
                      Print.printByOrder/printByOrderAll,
                      Eval.precision
* `gwamd.graph`     — owning handle over a gw_graph (edgelist / networkx /
                      R-MAT constructors)
* `gwamd.io`        — save_list / read_list / read_simrank formats
"""
from . import _lib
from ._lib import device_count, lib
from . import classify
from . import neighbors
from .graph import GWGraph

__all__ = ["GWGraph", "classify", "neighbors", "device_count", "lib", "_lib"]
__version__ = "0.1.0"
