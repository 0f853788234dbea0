"""forging-control_amd — MI355X-native (gfx950) unsupervised-MPC rollout engine.

Drop-in for the hot path of marcowus/forging-control: ``MPCLoss`` (the batched closed-loop rollout of
the FNN controller through the 3-layer LSTM plant surrogate, Functions.py:1336-1472) and its
backward, as hand-written HIP kernels behind the C ABI in include/fcr.h.
"""
from . import _native, closed_loop, data, distributed, graphed, inference, launch, loss_terms, many, mpc, plant, rollout, supervised, surrogate
from .functions import FNNModel, LSTMModel, MPCLoss, NeuralNetwork
from .inference import controller_step, simulate_rollout, simulate_step, simulator_make_step
from .plant import ForgingRK4, PressParams, fit_press, forging_rk4
from .data import DeviceLoader, SequenceWindows, free_run_batches
from .surrogate import free_run, train_free_run
from .closed_loop import ClosedLoop, ClosedLoopBank, FeasibilityRecovery
from .graphed import CapturedStep
from .many import ControllerBank, zip_loaders
from .loss_terms import LossTerms
from . import press_loss
from .press_loss import PressLoss, train_on_press
from .mpc import PressMPC, mpc_dataset

__all__ = ["press_loss", "PressLoss", "train_on_press","FNNModel", "LSTMModel", "MPCLoss", "NeuralNetwork", "rollout", "distributed", "inference",
           "simulate_step", "simulate_rollout", "controller_step", "simulator_make_step", "plant", "ForgingRK4", "forging_rk4", "PressParams", "fit_press",
           "data", "SequenceWindows", "DeviceLoader", "free_run_batches", "surrogate", "free_run", "train_free_run", "closed_loop", "ClosedLoop", "ClosedLoopBank", "FeasibilityRecovery", "graphed",
           "CapturedStep", "launch", "supervised", "many", "ControllerBank", "zip_loaders", "loss_terms", "LossTerms", "mpc", "PressMPC", "mpc_dataset", "_native"]
