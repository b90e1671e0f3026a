"""MI355X-native CTR training hot path of jqsl2012/RL_CTR_Prediction.

LR / FM / FFM / WideAndDeep / DeepFM / InnerPNN / OuterPNN / FNN / DCN / AFM / Feature_Embedding / PolicyGradient / the hybrid TD3
agent (Hybrid_TD3_Model, Critic, hybrid_actors) and its prioritized replay Memory with the
reference's construction API,
running on hand-written gfx950 HIP kernels behind the C ABI in include/ctr_hip.h
(libctr_hip.so). See DESIGN.md.
"""
from .afm_trainer import FusedAFMTrainer
from .feature_embedding import Feature_Embedding
from .ffm_trainer import FusedFFMTrainer
from .hybrid_td3_model_per import Critic, Hybrid_TD3_Model, hybrid_actors
from .metrics import DeviceMetrics, roc_auc_score
from .optim import DenseAdam
from .p_model import AFM, DCN, FFM, FM, FNN, LR, DeepFM, InnerPNN, OuterPNN, WideAndDeep
from .pg_model import Net, PolicyGradient
from .replay_memory import Memory as PrioritizedMemory
from .sharded import ShardedCTRTrainer
from .trainer import FusedCTRTrainer

__all__ = ["LR", "FM", "FFM", "WideAndDeep", "DeepFM", "InnerPNN", "OuterPNN", "FNN", "DCN", "AFM", "Feature_Embedding", "Net", "PolicyGradient", "FusedCTRTrainer",
           "FusedFFMTrainer", "FusedAFMTrainer", "ShardedCTRTrainer", "DenseAdam", "PrioritizedMemory",
           "Hybrid_TD3_Model", "Critic", "hybrid_actors", "DeviceMetrics", "roc_auc_score"]
