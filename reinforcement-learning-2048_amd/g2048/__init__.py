"""g2048: MI355X-native batched 2048 environment + Double-DQN hot path.

Drop-in for the hot path of ribal-aladeeb/reinforcement-learning-2048 (src/board.py,
src/dqn_lib.py): the env step, replay buffer and train_step, batched over tens of thousands of
boards per launch on gfx950.  Native code: csrc/g2048.hip -> libg2048.so (C ABI include/g2048.h).
"""
from ._native import NativeError, load as load_native  # noqa: F401
from . import (deepsearch, ntlambda, ntmean, ntmeantc, ntplay, ntrestart, ntsearch, ntstage,  # noqa: F401
               nttc, ntuple, search, stageback, stagedelay, stagemean, stagemeantc, stagesearch)
from .env import ACTIONS, EpisodeLog, ReplayBuffer, VecEnv2048, decode_episodes  # noqa: F401
from .search import (SearchWeights, expectimax,  # noqa: F401
                     generate_replay_buffer_using_expectimax)
from .ntuple import (TUPLES_2x4, TUPLES_4x6, NTupleNetwork, NTupleSpec,  # noqa: F401
                     NTupleTrainer)
from .nttc import TCState, TCTrainer  # noqa: F401
from .ntlambda import TDLambdaState, TDLambdaTrainer  # noqa: F401
from .ntstage import StagedNTupleNetwork  # noqa: F401
from .ntrestart import RestartPool  # noqa: F401
from .ntmean import MeanState, MeanTrainer, default_mean_lr_shift  # noqa: F401
from .stagemean import StagedMeanState, StagedMeanTrainer  # noqa: F401
from .ntmeantc import MeanTCState, MeanTCTrainer, default_meantc_lr_shift  # noqa: F401
from .stagemeantc import StagedMeanTCState, StagedMeanTCTrainer  # noqa: F401
from .stagedelay import DelayedLambdaState, DelayedLambdaTrainer  # noqa: F401
from .stageback import BackwardState, BackwardTrainer  # noqa: F401

__all__ = ["VecEnv2048", "ReplayBuffer", "EpisodeLog", "decode_episodes", "ACTIONS", "NativeError",
           "load_native", "search", "SearchWeights", "expectimax",
           "generate_replay_buffer_using_expectimax", "ntuple", "NTupleSpec", "NTupleNetwork",
           "NTupleTrainer", "TUPLES_4x6", "TUPLES_2x4", "ntsearch",
           "nttc", "TCState", "TCTrainer", "ntlambda", "TDLambdaState", "TDLambdaTrainer",
           "ntstage", "StagedNTupleNetwork", "stagesearch", "ntrestart", "RestartPool",
           "ntmean", "MeanState", "MeanTrainer", "default_mean_lr_shift",
           "stagemean", "StagedMeanState", "StagedMeanTrainer",
           "ntmeantc", "MeanTCState", "MeanTCTrainer", "default_meantc_lr_shift",
           "stagemeantc", "StagedMeanTCState", "StagedMeanTCTrainer", "deepsearch",
           "stagedelay", "DelayedLambdaState", "DelayedLambdaTrainer",
           "stageback", "BackwardState", "BackwardTrainer", "ntplay"]
