"""Drop-in `Wav2Letter` for speechless.configuration, backed by the MI355X engine.

Mirrors the API surface of the reference's speechless/net.py:117-607 as consumed by speechless/configuration.py
(:96-139,:159-215), main.py (:121,:144,:202) and README.md (:85,:119): same constructor signature, `predict`,
`test_and_predict`, `test_and_predict_batch(es)`, `test_and_predict_grouped_batches`, `predict_batch_greedily`,
`prediction_batch`, `train`, `load_weights`, attributes `predictive_net`, `grapheme_encoding`,
`input_to_prediction_length_ratio`, and the result types `ExpectationVsPrediction*` (net.py:22-114).

All arithmetic (11 x Conv1D, softmax, CTC loss/gradient, greedy decode, Adam) runs in hand-written gfx950 kernels via
speechless_amd.engine; this file is host plumbing (batch packing net.py:578-607, result objects, epoch loop).
"""
import logging
import sys
from collections import OrderedDict
from pathlib import Path

import numpy as np

from .engine import Engine, wav2letter_layer_specs
from .error_counts import edit_distance, space_index_of
from .grapheme_encoding import AsgGraphemeEncoding, CtcGraphemeEncoding

logger = logging.getLogger("results")
if not logger.handlers:
    logger.setLevel(logging.INFO)
    _handler = logging.StreamHandler(sys.stdout)
    _handler.setLevel(logging.INFO)
    logger.addHandler(_handler)


def log(obj):
    logger.info(str(obj))


def _average_or_nan(numbers):
    return sum(numbers) / len(numbers) if len(numbers) else float("nan")


class Adam:
    """Hyper-parameters of keras.optimizers.Adam as the reference constructs it (net.py:132: Adam(1e-4)), with what Keras
    2.0 lets a user add: Adam's own `decay` (lr / (1 + decay * iterations)) and the `clipnorm` / `clipvalue` every Keras
    optimizer accepts (global-norm scaling, then element clamp).  0 = off.  Restated from knowledge of Keras 2.0.x
    (optimizers.py), like the update itself; not checkable offline."""

    def __init__(self, lr=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.0, clipnorm=0.0, clipvalue=0.0):
        self.lr, self.beta_1, self.beta_2, self.epsilon = lr, beta_1, beta_2, epsilon
        self.decay, self.clipnorm, self.clipvalue = decay, clipnorm, clipvalue


class _KerasOptimizer:
    """what the optimizer classes below share: Keras 2.0's keyword names, plus the `decay`, `clipnorm` and `clipvalue` of Adam"""

    def __init__(self, lr, decay, clipnorm, clipvalue, **own):
        self.lr, self.decay, self.clipnorm, self.clipvalue = lr, decay, clipnorm, clipvalue
        for name, value in own.items():
            setattr(self, name, value)


class SGD(_KerasOptimizer):
    """keras.optimizers.SGD (2.0.x): v = momentum * m - lr * g; p += v (nesterov: p += momentum * v - lr * g)"""

    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False, clipnorm=0.0, clipvalue=0.0):
        super().__init__(lr, decay, clipnorm, clipvalue, momentum=momentum, nesterov=nesterov)


class RMSprop(_KerasOptimizer):
    """keras.optimizers.RMSprop (2.0.x): a = rho * a + (1 - rho) * g^2; p -= lr * g / (sqrt(a) + epsilon)"""

    def __init__(self, lr=0.001, rho=0.9, epsilon=1e-8, decay=0.0, clipnorm=0.0, clipvalue=0.0):
        super().__init__(lr, decay, clipnorm, clipvalue, rho=rho, epsilon=epsilon)


class Adagrad(_KerasOptimizer):
    """keras.optimizers.Adagrad (2.0.x): a += g^2; p -= lr * g / (sqrt(a) + epsilon)"""

    def __init__(self, lr=0.01, epsilon=1e-8, decay=0.0, clipnorm=0.0, clipvalue=0.0):
        super().__init__(lr, decay, clipnorm, clipvalue, epsilon=epsilon)


class Adadelta(_KerasOptimizer):
    """keras.optimizers.Adadelta (2.0.x): a = rho * a + (1 - rho) * g^2; u = g * sqrt(d + epsilon) / sqrt(a + epsilon);
    p -= lr * u; d = rho * d + (1 - rho) * u^2"""

    def __init__(self, lr=1.0, rho=0.95, epsilon=1e-8, decay=0.0, clipnorm=0.0, clipvalue=0.0):
        super().__init__(lr, decay, clipnorm, clipvalue, rho=rho, epsilon=epsilon)


class Adamax(_KerasOptimizer):
    """keras.optimizers.Adamax (2.0.x): m = beta_1 * m + (1 - beta_1) * g; u = max(beta_2 * u, |g|);
    p -= lr / (1 - beta_1^t) * m / (u + epsilon)"""

    def __init__(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.0, clipnorm=0.0, clipvalue=0.0):
        super().__init__(lr, decay, clipnorm, clipvalue, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon)


# class name -> (Engine `optimizer`, {Engine keyword: attribute read off the object}); only these attributes are read
_OPTIMIZER_RULES = {
    "SGD": ("sgd", {"momentum": "momentum", "nesterov": "nesterov"}),
    "RMSprop": ("rmsprop", {"rho": "rho", "adam_epsilon": "epsilon"}),
    "Adagrad": ("adagrad", {"adam_epsilon": "epsilon"}),
    "Adadelta": ("adadelta", {"rho": "rho", "adam_epsilon": "epsilon"}),
    "Adamax": ("adamax", {"beta_1": "beta_1", "beta_2": "beta_2", "adam_epsilon": "epsilon"}),
}


def optimizer_settings(optimizer):
    """The Engine keyword arguments an optimizer object stands for.  The rule is picked by the NAME of the object's class
    (a real Keras SGD / RMSprop / Adagrad / Adadelta / Adamax works like the classes above) and only that rule's attributes
    are read; any other class but Nadam is read as Adam always was: lr, beta_1, beta_2, epsilon,
    and decay / clipnorm / clipvalue where the object has them (a Keras optimizer carries clipnorm / clipvalue only when
    they were given: absent = 0 = off)."""
    extra = {name: float(getattr(optimizer, name, 0.0) or 0.0) for name in ("decay", "clipnorm", "clipvalue")}
    name = type(optimizer).__name__
    if name in _OPTIMIZER_RULES:
        rule, attributes = _OPTIMIZER_RULES[name]
        own = {keyword: getattr(optimizer, attribute) for keyword, attribute in attributes.items()}
        return dict(optimizer=rule, lr=optimizer.lr, **own, **extra)
    supported = "Adam, " + ", ".join(_OPTIMIZER_RULES)
    if name == "Nadam":
        raise ValueError("Nadam is not supported (its momentum schedule is host state of another kind); the optimizers are "
                         + supported)
    if not all(hasattr(optimizer, a) for a in ("lr", "beta_1", "beta_2", "epsilon")):
        raise ValueError("unknown optimizer class {!r}: the supported optimizers are {}".format(name, supported))
    return dict(lr=optimizer.lr, beta_1=optimizer.beta_1, beta_2=optimizer.beta_2, adam_epsilon=optimizer.epsilon, **extra)


def optimizer_state_to_arrays(state, layer_names):
    """Engine.get_optimizer_state() as the flat {name: array} dictionary of a weights-epoch{N}.opt.npz file: the rule's name
    (left out for Adam: its files are what they always were) and, per layer, the slots the rule has ('m', and 'v' for a
    two-slot rule)"""
    arrays = {"iterations": np.int64(state["iterations"]), "dropout_steps": np.int64(state["dropout_steps"])}
    if state.get("optimizer", "adam") != "adam":
        arrays["optimizer"] = np.array(state["optimizer"])
    for slot in ("m", "v"):
        if slot in state:
            for name, (w, b) in zip(layer_names, state[slot]):
                arrays["{}/kernel/{}".format(name, slot)], arrays["{}/bias/{}".format(name, slot)] = w, b
    return arrays


def optimizer_state_from_arrays(data, layer_names):
    """the reverse (data: an opened .npz or a dictionary); a file without the rule's name is an Adam state"""
    rule = str(data["optimizer"]) if "optimizer" in data else "adam"
    state = {"iterations": int(data["iterations"]), "dropout_steps": int(data["dropout_steps"])}
    if rule != "adam":
        state["optimizer"] = rule
    for slot in ("m", "v"):
        if "{}/kernel/{}".format(layer_names[0], slot) in data:
            state[slot] = [(data["{}/kernel/{}".format(n, slot)], data["{}/bias/{}".format(n, slot)]) for n in layer_names]
    return state


class LabeledSpectrogram:
    """Duck type of speechless.labeled_example.LabeledSpectrogram (labeled_example.py:63-71)."""

    def __init__(self, id, label, spectrogram=None):
        self.id = id
        self.label = label
        self._spectrogram = spectrogram

    def z_normalized_transposed_spectrogram(self):
        return self._spectrogram


class ExpectationVsPrediction:
    def __init__(self, expected, predicted, loss, letter_error_count=None, word_error_count=None):
        """letter_error_count / word_error_count (extension): counts that were taken elsewhere -- on the GPU,
        Wav2Letter(error_count_device="gpu") -- stored as they are; None computes them here as the reference does."""
        self.expected = expected
        self.predicted = predicted
        self.loss = loss
        self.expected_letter_count = len(expected)
        self.expected_words = expected.split()
        self.expected_word_count = len(self.expected_words)
        self.letter_error_count = edit_distance(expected, predicted) if letter_error_count is None \
            else letter_error_count
        self.word_error_count = edit_distance(self.expected_words, predicted.split()) if word_error_count is None \
            else word_error_count

    @property
    def letter_error_rate(self):
        return self.letter_error_count / self.expected_letter_count

    @property
    def word_error_rate(self):
        return self.word_error_count / self.expected_word_count

    def __str__(self):
        return 'Expected:  "{}"\nPredicted: "{}"\nErrors: {} letters ({}%), {} words ({}%), loss: {:.2f}.'.format(
            self.expected, self.predicted, self.letter_error_count, round(self.letter_error_rate * 100),
            self.word_error_count, round(self.word_error_rate * 100), self.loss)


class ExpectationsVsPredictions:
    def __init__(self, results):
        self.results = results

    @property
    def average_letter_error_count(self):
        return _average_or_nan([r.letter_error_count for r in self.results])

    @property
    def average_word_error_count(self):
        return _average_or_nan([r.word_error_count for r in self.results])

    @property
    def average_letter_error_rate(self):
        return _average_or_nan([r.letter_error_rate for r in self.results])

    @property
    def average_word_error_rate(self):
        return _average_or_nan([r.word_error_rate for r in self.results])

    @property
    def average_loss(self):
        return _average_or_nan([r.loss for r in self.results])

    def summary_line(self):
        return ("Average over {} examples: {:.1f} letter errors ({:.2f}%), {:.1f} word errors ({:.2f}%), "
                "loss {:.2f}.").format(len(self.results), self.average_letter_error_count,
                                       self.average_letter_error_rate * 100, self.average_word_error_count,
                                       self.average_word_error_rate * 100, self.average_loss)

    def __str__(self):
        return "\n\n".join(str(r) for r in self.results) + "\n\n" + self.summary_line() + "\n\n"


class ExpectationsVsPredictionsInBatches(ExpectationsVsPredictions):
    def __init__(self, result_batches):
        self.result_batches = result_batches
        super().__init__([r for batch in result_batches for r in batch.results])

    def __str__(self):
        return "All batches: {}".format(self.summary_line())


class ExpectationsVsPredictionsInGroupedBatches(ExpectationsVsPredictions):
    def __init__(self, results_by_group_name):
        self.result_batches_by_group_name = results_by_group_name
        super().__init__([r for batches in results_by_group_name.values() for r in batches.results])

    def __str__(self):
        groups = "\n".join("{}: {}".format(name, batches)
                           for name, batches in self.result_batches_by_group_name.items())
        return "\n\n{}\n\nAll corpora: {}\n\n".format(groups, self.summary_line())


class _ConvLayerHandle:
    """What `predictive_net.layers[i]` needs to offer for net.py:237-269 style weight surgery."""

    def __init__(self, net, index, name):
        self._net, self._index, self.name = net, index, name
        self.trainable = True

    def get_weights(self):
        return list(self._net.get_weights()[self._index])

    def set_weights(self, kernel_and_bias):
        weights = self._net.get_weights()
        weights[self._index] = (np.asarray(kernel_and_bias[0], dtype=np.float32),
                                np.asarray(kernel_and_bias[1], dtype=np.float32))
        self._net.set_weights(weights)


class PredictiveNet:
    """Stand-in for the Keras Sequential the reference exposes as `Wav2Letter.predictive_net` (net.py:168)."""

    def __init__(self, engine):
        self._engine = engine
        self.layers = [_ConvLayerHandle(self, i, s.name) for i, s in enumerate(engine.all_specs)]

    def get_weights(self):
        return self._engine.get_weights()

    def set_weights(self, weights):
        self._engine.set_weights(weights)

    def save_weights(self, path):
        """Keras writes HDF5 (net.py:572: `predictive_net.save_weights(...)`): the same file -- root attribute
        `layer_names`, one group per layer with `weight_names`, `<layer>/kernel:0` (k, Cin, Cout) and `<layer>/bias:0`
        below it -- through speechless_amd/h5lite.py (no h5py needed; the real HDF5 library reads it, tests/test_h5lite.py).
        A path ending in .npz keeps the flat numpy form (`<layer>/kernel`, `<layer>/bias`)."""
        path = Path(path)
        weights = self.get_weights()
        if path.suffix == ".npz":
            arrays = {}
            for layer, (w, b) in zip(self.layers, weights):
                arrays[layer.name + "/kernel"] = w
                arrays[layer.name + "/bias"] = b
            np.savez(str(path), **arrays)
            return
        from . import h5lite
        h5lite.write_keras_weights(path, [(layer.name, [("{}/kernel:0".format(layer.name), w),
                                                         ("{}/bias:0".format(layer.name), b)])
                                          for layer, (w, b) in zip(self.layers, weights)])

    def load_weights(self, path):
        """Loads a Keras HDF5 checkpoint of the reference (`weights-epoch{N}.h5` from `save_weights`, net.py:209-212, or a
        full-model file whose tree sits under `model_weights`; Keras-1 weight names `<layer>_W` / `<layer>_b` and
        (k, 1, Cin, Cout) kernels included), or the flat .npz form.  When the .h5 that was asked for does not exist but
        its `.npz` twin does (files written by round-1/2 versions of this class), that one is used -- and logged."""
        path = Path(path)
        npz = path.with_suffix(".npz")
        if path.suffix == ".npz" or (not path.exists() and npz.exists()):
            if path.suffix != ".npz":
                log("{} not found: loading {}".format(path.name, npz.name))
            data = np.load(str(npz))
            self.set_weights([(data[layer.name + "/kernel"], data[layer.name + "/bias"]) for layer in self.layers])
            return
        from . import h5lite
        by_name = dict(h5lite.read_keras_weights(path))
        weights = []
        for layer in self.layers:
            if layer.name not in by_name:
                raise ValueError("{} holds no weights for layer {!r} (layers with weights: {})".format(
                    path.name, layer.name, ", ".join(by_name)))
            entry = by_name[layer.name]
            kernel = [v for n, v in entry.items() if "kernel" in n or n.endswith("W:0") or n.endswith("_W")]
            bias = [v for n, v in entry.items() if "bias" in n or n.endswith("b:0") or n.endswith("_b")]
            if len(kernel) != 1 or len(bias) != 1:
                raise ValueError("layer {!r} of {}: expected one kernel and one bias, found {}".format(
                    layer.name, path.name, list(entry)))
            w = np.asarray(kernel[0])
            if w.ndim == 4:  # Keras-1 style conv kernels (k, 1, Cin, Cout)
                w = w.reshape(w.shape[0], w.shape[2], w.shape[3])
            weights.append((w, np.asarray(bias[0])))
        self.set_weights(weights)


class Wav2Letter:
    """Speech-recognition network based on wav2letter (https://arxiv.org/pdf/1609.03193v2.pdf), MI355X engine."""

    class InputNames:
        input_batch = "input_batch"
        label_batch = "label_batch"
        prediction_lengths = "prediction_lenghts"  # (sic) reference net.py:123
        label_lengths = "label_lenghts"  # (sic) reference net.py:124

    def __init__(self, input_size_per_time_step, allowed_characters, use_raw_wave_input=False, activation="relu",
                 output_activation="softmax", optimizer=None, dropout=None, load_model_from_directory=None,
                 load_epoch=None, allowed_characters_for_loaded_model=None, frozen_layer_count=0,
                 reinitialize_trainable_loaded_layers=False, use_asg=False, asg_transition_probabilities=None,
                 asg_initial_probabilities=None, kenlm_directory=None,
                 # --- extensions of this implementation (keyword-only in spirit) ---
                 compute_dtype=None, device="cuda:0", seed=None, ctc_epsilon=1e-8, layer_sizes=None,
                 load_optimizer_state=False, eval_dtype=None, beam_search_device="host", track_gradient_norm=False,
                 error_count_device="host", criterion="ctc"):
        if frozen_layer_count > 0 and load_model_from_directory is None:
            raise ValueError("Layers cannot be frozen if model is trained from scratch.")
        if use_asg:
            raise NotImplementedError("ASG is not yet implemented.")  # as reference net.py:396-399
        # extension: criterion="asg" is this implementation's ASG (csrc/asg.hip; DESIGN.md "ASG criterion") -- use_asg keeps
        # raising as the reference does.  "asg" reads asg_transition_probabilities / asg_initial_probabilities (ignored
        # under "ctc", as ever), encodes labels with AsgGraphemeEncoding (K = characters + 2, no blank), trains and
        # evaluates with the ASG loss and decodes by the Viterbi path over emissions + transition scores.
        if criterion not in ("ctc", "asg"):
            raise ValueError("criterion must be 'ctc' or 'asg', not {!r}".format(criterion))
        self.criterion = criterion
        if criterion == "asg":
            if kenlm_directory is not None and beam_search_device != "gpu":
                raise ValueError("criterion='asg': kenlm_directory needs beam_search_device='gpu' (asg_beam.hip); there is "
                                 "no host ASG beam search")
            clipped = optimizer is not None and optimizer_settings(optimizer)
            if track_gradient_norm or (clipped and (clipped["clipnorm"] or clipped["clipvalue"])):
                raise ValueError("criterion='asg': gradient clipping (clipnorm / clipvalue) and track_gradient_norm cover the "
                                 "conv stack's gradients only, not the ASG tables; not supported")
        if dropout is not None and not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must be a rate in [0, 1)")
        self.kenlm_directory = kenlm_directory
        if beam_search_device not in ("host", "gpu"):
            raise ValueError("beam_search_device must be 'host' or 'gpu', not {!r}".format(beam_search_device))
        self.beam_search_device = beam_search_device
        if error_count_device not in ("host", "gpu"):
            raise ValueError("error_count_device must be 'host' or 'gpu', not {!r}".format(error_count_device))
        self.error_count_device = error_count_device
        # extension: "gpu" takes the letter / word error counts of test_and_predict_batch from csrc/edit_distance.hip
        self._space_index = space_index_of(allowed_characters) if error_count_device == "gpu" else None
        self.grapheme_encoding = (AsgGraphemeEncoding if criterion == "asg" else CtcGraphemeEncoding)(
            allowed_characters=allowed_characters)
        self.use_asg = use_asg
        self.frozen_layer_count = frozen_layer_count
        self.output_activation = output_activation
        self.activation = activation
        self.use_raw_wave_input = use_raw_wave_input
        self.input_size_per_time_step = input_size_per_time_step
        self.optimizer = optimizer if optimizer is not None else Adam(1e-4)
        self.load_epoch = load_epoch
        self.dropout = dropout
        # Arithmetic (round 6).  The reference has ONE arithmetic -- fp32 (net.py:389,402-406).  Called with
        # the reference's own signature (compute_dtype not given) this class TRAINS on the benchmarked bf16 engine and
        # EVALUATES -- prediction_batch, predict*, test_and_predict* -- on a second, lazily built engine of a fast PARITY
        # path (greedy decode bit-exact against the fp32 CPU port, loss to 2e-7) that shares the fp32 master weights in HBM
        # and re-packs its operand copies whenever they changed: `f16x3` (hi + lo fp16 planes, 22 operand bits; weights
        # representable up to |w| < 1000 -- eval_engine falls back to bf16x3 beyond that) for spectrogram input, `bf16x3`
        # (hi + lo bf16 planes, fp32's range) for raw-wave input -- which runs on `f16x3` too when asked for by name
        # (eval_dtype / compute_dtype; samples stored scaled by Engine.x_scale, _check_sample_range).  compute_dtype="bf16" / "f32" / "bf16x3" / "f16x3" given
        # explicitly: that one engine does everything (eval_dtype overrides the evaluation side alone).
        self.compute_dtype = compute_dtype if compute_dtype is not None else "bf16"
        if eval_dtype is None:
            eval_dtype = ("bf16x3" if use_raw_wave_input else "f16x3") if compute_dtype is None else self.compute_dtype
        self.eval_dtype = eval_dtype
        compute_dtype = self.compute_dtype
        self.device = device
        self.ctc_epsilon = ctc_epsilon
        self._layer_sizes = dict(layer_sizes or {})
        specs = wav2letter_layer_specs(input_size_per_time_step, self.grapheme_encoding.grapheme_set_size,
                                       activation=activation, output_activation=output_activation,
                                       use_raw_wave_input=use_raw_wave_input, **self._layer_sizes)
        self.engine = Engine(specs, self.grapheme_encoding.grapheme_set_size, dtype=compute_dtype, device=device,
                             ctc_epsilon=ctc_epsilon, frozen_layer_count=frozen_layer_count,
                             track_grad_norm=track_gradient_norm, criterion=criterion, **optimizer_settings(self.optimizer))
        if criterion == "asg":
            self.engine.set_asg_scores(*self._asg_scores(asg_transition_probabilities, asg_initial_probabilities,
                                                         self.grapheme_encoding.grapheme_set_size, ctc_epsilon))
        self.engine.dropout_rate = dropout if dropout else None  # applied by training steps only (learning phase 1)
        # the reference signature has no seed: a plain Wav2Letter(..., dropout=0.1) draws one (Keras does the same)
        self.engine.dropout_seed = int(seed) if seed is not None else \
            int(np.random.SeedSequence().entropy & 0x7fffffff)
        self.engine.set_weights(self._glorot_uniform(specs, seed))
        self._eval_engine = None
        self._eval_weights_version = None
        self.predictive_net = PredictiveNet(self.engine)
        for layer in self.predictive_net.layers[:frozen_layer_count]:
            layer.trainable = False
        if frozen_layer_count > 0:
            log("All but {} layers frozen.".format(len(specs) - frozen_layer_count))
        self.prediction_phase_flag = 0.
        self._beam_decoder = None
        if self.kenlm_directory is not None:  # net.py:171-177
            from .decoder import CtcBeamSearchDecoder, expected_characters
            expected = expected_characters(self.kenlm_directory)
            if list(allowed_characters) != expected:
                raise ValueError("Allowed characters {} differ from those expected by kenlm decoder: {}".format(
                    allowed_characters, expected))
            if criterion == "asg":  # extension: the ASG beam search of asg_beam.hip (Engine.asg_beam_search)
                from .decoder import GpuAsgBeamSearchDecoder
                self._beam_decoder = GpuAsgBeamSearchDecoder.from_kenlm_directory(
                    self.kenlm_directory, allowed_characters, device=device)
            elif beam_search_device == "gpu":  # extension: the same search in ctc_beam.hip (Engine.beam_search)
                from .decoder import GpuCtcBeamSearchDecoder
                self._beam_decoder = GpuCtcBeamSearchDecoder.from_kenlm_directory(
                    self.kenlm_directory, allowed_characters, epsilon=ctc_epsilon, device=device)
            else:
                self._beam_decoder = CtcBeamSearchDecoder.from_kenlm_directory(self.kenlm_directory, allowed_characters,
                                                                               epsilon=ctc_epsilon)
        if load_model_from_directory is not None:
            self.load_weights(allowed_characters_for_loaded_model, load_epoch, load_model_from_directory,
                              loaded_first_layers_count=frozen_layer_count if reinitialize_trainable_loaded_layers
                              else None)
            if load_optimizer_state:
                self.load_optimizer_state(load_model_from_directory, load_epoch)

    @staticmethod
    def _glorot_uniform(specs, seed):
        """Keras default initialisers: glorot_uniform kernels (limit sqrt(6/(fan_in+fan_out))), zero biases."""
        rng = np.random.RandomState(seed)
        weights = []
        for s in specs:
            limit = np.sqrt(6.0 / (s.kernel_size * s.cin + s.kernel_size * s.cout))
            weights.append((rng.uniform(-limit, limit, size=(s.kernel_size, s.cin, s.cout)).astype(np.float32),
                            np.zeros((s.cout,), dtype=np.float32)))
        return weights

    @staticmethod
    def _asg_scores(transition_probabilities, initial_probabilities, k, eps):
        """The ASG tables a net starts from: log(P + eps) of the given probabilities -- (K, K) [from][to] and (K,), or the
        (K + 1, K + 1) / (K + 1,) form of the reference's defaults with row, column and entry 0 dropped (net.py:274-277,
        285-286) -- and all-zero scores for None, the initialisation of the wav2letter paper.  (The reference's own default
        is an unseeded random draw, net.py:273 / :285, that nothing can reproduce: it is not imitated.)"""
        def scores(p, shape, what):
            if p is None:
                return np.zeros(shape, dtype=np.float32)
            p = np.asarray(p, dtype=np.float64)
            if p.shape == tuple(n + 1 for n in shape):
                p = p[(slice(1, None),) * len(shape)]
            if p.shape != shape or (p < 0).any():
                raise ValueError("{} must be non-negative with shape {} (or one larger: the reference's form with index 0 "
                                 "unused), got shape {}".format(what, shape, p.shape))
            return np.log(p + eps).astype(np.float32)
        return (scores(transition_probabilities, (k, k), "asg_transition_probabilities"),
                scores(initial_probabilities, (k,), "asg_initial_probabilities"))

    # ------------------------------------------------------------------ weights (net.py:184-269, 558-560)
    @staticmethod
    def model_file_name(epoch):
        return "weights-epoch{}.h5".format(epoch)

    @staticmethod
    def asg_file_name(epoch):
        return "asg-epoch{}.npz".format(epoch)

    def save_asg_state(self, net_directory, epoch):
        """criterion="asg": the transition scores, the start scores and their Adam moments, beside the weights file"""
        Path(net_directory).mkdir(parents=True, exist_ok=True)
        np.savez(str(Path(net_directory) / self.asg_file_name(epoch)), **self.engine.get_asg_state())

    def _load_asg_state(self, net_directory, epoch, with_moments):
        """reads asg-epoch{N}.npz when the net is an ASG net and the file is there (a CTC checkpoint has none)"""
        path = Path(net_directory) / self.asg_file_name(epoch)
        if self.criterion != "asg" or not path.exists():
            return
        data = np.load(str(path))
        names = [n for n in data.files if with_moments or n in ("trans", "init")]
        self.engine.set_asg_state({n: data[n] for n in names})

    @staticmethod
    def optimizer_state_file_name(epoch):
        return "weights-epoch{}.opt.npz".format(epoch)

    def save_optimizer_state(self, net_directory, epoch):
        """Extension: the reference saves the weights only (net.py:564-572), so a resumed run
        restarts Adam's moments and bias correction.  This writes them next to the weights file of the same epoch."""
        arrays = optimizer_state_to_arrays(self.engine.get_optimizer_state(), [l.name for l in self.predictive_net.layers])
        Path(net_directory).mkdir(parents=True, exist_ok=True)
        np.savez(str(Path(net_directory) / self.optimizer_state_file_name(epoch)), **arrays)

    def load_optimizer_state(self, net_directory, epoch):
        self._load_asg_state(net_directory, epoch, with_moments=True)
        data = np.load(str(Path(net_directory) / self.optimizer_state_file_name(epoch)))
        self.engine.set_optimizer_state(optimizer_state_from_arrays(data, [l.name for l in self.predictive_net.layers]))

    @staticmethod
    def indices_to_load_by_target_index(allowed_characters_for_loaded_model, allowed_characters):
        ignored = set(allowed_characters_for_loaded_model) - set(allowed_characters)
        if ignored:
            log("Ignoring characters {} from loaded model.".format(sorted(ignored)))
        extra = set(allowed_characters) - set(allowed_characters_for_loaded_model)
        if extra:
            log("Initializing extra characters {} not found in model.".format(sorted(extra)))
        mapping = []
        for character in allowed_characters:
            hits = [i for i, c in enumerate(allowed_characters_for_loaded_model) if c == character]
            assert len(hits) <= 1
            mapping.append(hits[0] if hits else None)
        log("Character mapping: {}".format(mapping))
        return mapping

    def load_weights(self, allowed_characters_for_loaded_model, load_epoch, load_model_from_directory,
                     loaded_first_layers_count=None):
        path = Path(load_model_from_directory) / self.model_file_name(load_epoch)
        if allowed_characters_for_loaded_model is None:
            self.predictive_net.load_weights(path)
            self._load_asg_state(load_model_from_directory, load_epoch, with_moments=False)
            return
        if self.criterion == "asg":
            raise ValueError("criterion='asg': re-mapping a loaded model's characters (allowed_characters_for_loaded_model) "
                             "follows the CTC blank; not supported")
        layer_count = len(self.predictive_net.layers)
        if loaded_first_layers_count is None:
            loaded_first_layers_count = layer_count
        original = Wav2Letter(self.input_size_per_time_step, allowed_characters_for_loaded_model,
                              activation=self.activation, output_activation=self.output_activation,
                              optimizer=self.optimizer, load_model_from_directory=load_model_from_directory,
                              load_epoch=load_epoch, frozen_layer_count=self.frozen_layer_count,
                              compute_dtype=self.compute_dtype, device=self.device, layer_sizes=self._layer_sizes,
                              use_raw_wave_input=self.use_raw_wave_input)
        log("Loading first {} layers of {}, epoch {}, reinitializing the last {}.".format(
            loaded_first_layers_count, load_model_from_directory, load_epoch, layer_count - loaded_first_layers_count))
        source = original.predictive_net.get_weights()
        target = self.predictive_net.get_weights()
        for index in range(loaded_first_layers_count):
            kernel, bias = source[index]
            if index == layer_count - 1:
                mapping = self.indices_to_load_by_target_index(allowed_characters_for_loaded_model,
                                                               self.grapheme_encoding.allowed_characters)
                columns, biases = [], []
                for target_index in range(self.grapheme_encoding.grapheme_set_size):
                    source_index = original.grapheme_encoding.ctc_blank \
                        if target_index == self.grapheme_encoding.ctc_blank else mapping[target_index]
                    # reference quirk kept on purpose (net.py:254,258): `if index` also treats index 0 as missing
                    if source_index:
                        columns.append(kernel[:, :, source_index:source_index + 1])
                        biases.append(bias[source_index])
                    else:
                        columns.append(np.zeros((kernel.shape[0], kernel.shape[1], 1), dtype=kernel.dtype))
                        biases.append(0)
                kernel = np.concatenate(columns, axis=2)
                bias = np.array(biases, dtype=np.float32)
            target[index] = (kernel, bias)
        self.predictive_net.set_weights(target)

    # ------------------------------------------------------------------ packing (net.py:343-348, 578-607)
    @property
    def input_to_prediction_length_ratio(self):
        ratio = 1
        for s in self.engine.all_specs:
            ratio *= s.stride
        return ratio

    def _input_batch_and_prediction_lengths(self, spectrograms):
        input_lengths = [s.shape[0] for s in spectrograms]
        prediction_lengths = [n // self.input_to_prediction_length_ratio for n in input_lengths]
        input_batch = np.zeros((len(spectrograms), max(input_lengths), spectrograms[0].shape[1]), dtype=np.float32)
        for row, s in zip(input_batch, spectrograms):
            row[:s.shape[0], :s.shape[1]] = s
        self._check_sample_range(input_batch)
        return input_batch, prediction_lengths

    F16X3_SAMPLE_LIMIT = 6.0e4

    def _check_sample_range(self, input_batch):
        """Raw-wave input on f16x3: the sample windows are fp16 planes of x_scale * x (Engine.x_scale), which saturate at
        65504 -- a host batch beyond the range is refused here, before it is uploaded."""
        if not self.use_raw_wave_input or "f16x3" not in (self.compute_dtype, self.eval_dtype):
            return
        # (the evaluation engine is built lazily: until then its default scale stands in for it)
        x_scale = max((e.x_scale for e in (self.engine, self._eval_engine) if e is not None and e.x3_f16), default=1024.0)
        peak = float(np.abs(input_batch).max()) if input_batch.size else 0.0
        if not peak * x_scale < self.F16X3_SAMPLE_LIMIT:
            raise ValueError("raw-wave input on f16x3: max|x| * x_scale = {:g} * {:g} is not below the limit {:g} of the "
                             "fp16 sample planes (audio is expected in [-1, 1])".format(peak, x_scale, self.F16X3_SAMPLE_LIMIT))

    def _input_dictionary_for_loss_net(self, labeled_spectrogram_batch):
        spectrograms = [x.z_normalized_transposed_spectrogram() for x in labeled_spectrogram_batch]
        labels = [x.label for x in labeled_spectrogram_batch]
        input_batch, prediction_lengths = self._input_batch_and_prediction_lengths(spectrograms)
        n = len(labeled_spectrogram_batch)
        return {
            Wav2Letter.InputNames.input_batch: input_batch,
            Wav2Letter.InputNames.prediction_lengths: np.reshape(np.array(prediction_lengths), (n, 1)),
            Wav2Letter.InputNames.label_batch: self.grapheme_encoding.encode_label_batch(labels),
            Wav2Letter.InputNames.label_lengths: np.reshape(self._label_lengths(labels), (n, 1)),
        }

    def _label_lengths(self, labels):
        """graphemes per label: its characters -- under ASG its ENCODED length (a repeat mark replaces one or two letters)"""
        if self.criterion == "asg":
            return np.array([len(self.grapheme_encoding.encode(l)) for l in labels], dtype=np.int32)
        return np.array([len(l) for l in labels], dtype=np.int32)

    # ------------------------------------------------------------------ inference (net.py:350-357, 461-498)
    @property
    def eval_engine(self):
        """The engine every forward-only entry point runs on (net.py:350-357, 461-498: learning phase 0).  Same object as
        self.engine when training and evaluation share a dtype; otherwise a second Engine of self.eval_dtype over the SAME
        flat fp32 master buffer (no copy: `params` is aliased), whose packed operand copies are refreshed when the training
        engine's weights_version moved (a training step, set_weights, a loaded checkpoint)."""
        if self.eval_dtype == self.compute_dtype:
            return self.engine
        train = self.engine
        if self._eval_engine is None:
            ev = Engine(list(train.all_specs), self.grapheme_encoding.grapheme_set_size, dtype=self.eval_dtype,
                        device=self.device, ctc_epsilon=self.ctc_epsilon, frozen_layer_count=self.frozen_layer_count,
                        forward_only=True, criterion=self.criterion)
            ev.params = train.params  # the masters themselves: same plan, same offsets
            ev.asg_params = train.asg_params  # (None under CTC; the ASG tables are read in place, never packed)
            assert ev.param_numel == train.param_numel
            self._eval_engine = ev
            self._eval_weights_version = None
        ev = self._eval_engine
        if self._eval_weights_version != train.weights_version:
            if ev.x3_f16 and float(train.params.abs().max().item()) * ev.w_scale >= 6.0e4:
                # fp16 planes hold w_scale * w: a master beyond +-937 would saturate -- evaluate on bf16 planes instead
                log("weights beyond the range of the f16x3 evaluation path: evaluating on bf16x3")
                self.eval_dtype, self._eval_engine = "bf16x3", None
                return self.eval_engine
            ev._packed_dirty = True  # (its next forward re-packs from the shared masters, on the same stream as the step)
            self._eval_weights_version = train.weights_version
        return ev

    def prediction_batch(self, input_batch):
        """Grapheme probabilities (B, T', K) for a (B, T, F) spectrogram batch."""
        input_batch = np.asarray(input_batch)
        self._check_sample_range(input_batch)
        return self.eval_engine.forward(input_batch).cpu().numpy()

    def predict_batch_greedily(self, spectrograms):
        input_batch, prediction_lengths = self._input_batch_and_prediction_lengths(spectrograms)
        engine = self.eval_engine
        engine.forward(input_batch)
        decoded, _ = self._decode(engine, prediction_lengths)
        return [self.grapheme_encoding.decode_graphemes(d, merge_repeated=False) for d in decoded]

    def _decode(self, engine, prediction_lengths=None):
        """greedy CTC decode, or under ASG the Viterbi path with repeats merged (each grapheme is then decoded with its
        predecessor: AsgGraphemeEncoding.decode_graphemes)"""
        if self.criterion == "asg":
            return engine.asg_viterbi(prediction_lengths)
        return engine.greedy_decode(prediction_lengths)

    def _decode_for_evaluation(self, engine, prediction_lengths, lengths_are_set=False):
        """what test_and_predict_batch predicts from the engine's current forward pass: the beam search of the net's decoder if
        it has one (kenlm_directory), else _decode.  lengths_are_set: set_labels has stated the prediction lengths already."""
        if self._beam_decoder is not None and self.criterion == "asg":
            decoded, _ = engine.asg_beam_search(self._beam_decoder, prediction_lengths)
        elif self._beam_decoder is not None and self.beam_search_device == "gpu":
            decoded, _ = engine.beam_search(self._beam_decoder, prediction_lengths)
        elif self._beam_decoder is not None:  # net.py:444-451: beam search scored by the language model
            decoded, _ = self._beam_decoder.decode(engine.cur.probs.cpu().numpy(), prediction_lengths)
        else:
            decoded, _ = self._decode(engine, None if lengths_are_set else prediction_lengths)
        return decoded

    def predict_batch_greedily_from_audio(self, raw_audio_batch, sample_rate=16000, fourier_window_length=512,
                                          hop_length=128, original_sample_rates=None):
        """Extension: predict_batch_greedily for raw audio (1-D float arrays).  STFT, power level, mel projection and
        z-normalisation (labeled_example.py:99-160, 28-29) run on the GPU (speechless_amd/spectrogram.py) and their result
        feeds the conv stack directly in HBM -- no spectrogram crosses PCIe.
        original_sample_rates: one rate per utterance; those that differ from `sample_rate` are converted in HBM first
        (speechless_amd/resample.py: one launch per distinct rate), the others never pass through the filter."""
        from .spectrogram import shared_extractor
        bins = 1 + fourier_window_length // 2
        mel = None if self.input_size_per_time_step == bins else self.input_size_per_time_step
        extractor = shared_extractor(sample_rate, fourier_window_length, hop_length, mel, self.device)
        if original_sample_rates is not None and any(int(r) != sample_rate for r in original_sample_rates):
            x, frames = self._front_end_at_mixed_rates(extractor, raw_audio_batch, original_sample_rates)
        else:
            x, frames = extractor.batch(raw_audio_batch)
        engine = self.eval_engine
        engine.forward(x)
        decoded, _ = self._decode(engine, [n // self.input_to_prediction_length_ratio for n in frames])
        return [self.grapheme_encoding.decode_graphemes(d, merge_repeated=False) for d in decoded]

    @staticmethod
    def _front_end_at_mixed_rates(extractor, raw_audio_batch, rates):
        """extractor.batch() for utterances at their own sample rates: the samples cross PCIe as they are, the converted
        utterances are written behind them in the same device buffer and the front end reads each where it then lies."""
        import torch
        from .resample import MixedRatePlan
        audios = [np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.float32) for a in raw_audio_batch]
        if not audios or min(a.shape[0] for a in audios) < 1:
            raise ValueError("empty batch or empty audio")
        lengths = np.array([a.shape[0] for a in audios], dtype=np.int32)
        offsets = np.zeros(len(audios), dtype=np.int64)
        offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
        n = int(lengths.sum(dtype=np.int64))
        plan = MixedRatePlan(offsets, lengths, rates, extractor.sample_rate, n)
        if plan.lengths.min() <= extractor.n_fft // 2:
            raise ValueError("audio shorter than {} samples cannot be reflect-padded (librosa.stft raises too)".format(
                extractor.n_fft // 2 + 1))
        device = extractor.device
        buffer = torch.empty((plan.total,), dtype=torch.float32, device=device)
        buffer[:n].copy_(torch.from_numpy(np.concatenate(audios)))
        plan.launch(plan.to_device(device), buffer, device)
        return extractor.batch_device(buffer, torch.from_numpy(plan.offsets).to(device),
                                      torch.from_numpy(plan.lengths).to(device), plan.lengths)

    def test_and_predict_batch(self, labeled_spectrogram_batch):
        """ONE forward pass yields both the greedy transcription and the per-utterance CTC loss."""
        inputs = self._input_dictionary_for_loss_net(labeled_spectrogram_batch)
        names = Wav2Letter.InputNames
        engine = self.eval_engine
        engine.forward(inputs[names.input_batch])
        engine.set_labels(inputs[names.label_batch], inputs[names.label_lengths],
                          inputs[names.prediction_lengths])
        losses = engine.loss().cpu().numpy()
        decoded = self._decode_for_evaluation(engine, inputs[names.prediction_lengths], lengths_are_set=True)
        predictions = [self.grapheme_encoding.decode_graphemes(d, merge_repeated=False) for d in decoded]
        n = len(predictions)
        letter_errors = word_errors = [None] * n  # None: ExpectationVsPrediction counts on the host (net.py:31-37)
        if self.error_count_device == "gpu" and self._beam_decoder is None:  # labels and `decoded` are in HBM already
            letter_errors, word_errors = (c.tolist() for c in engine.error_counts(self._space_index))
        elif self.error_count_device == "gpu":
            label_lengths = inputs[names.label_lengths].reshape(-1)
            expected = [row[:m].tolist() for row, m in zip(inputs[names.label_batch], label_lengths)]
            letter_errors, word_errors = (c.tolist() for c in engine.edit_distance_batch(expected, decoded, self._space_index))
        return ExpectationsVsPredictions(
            [ExpectationVsPrediction(predicted=p, expected=x.label, loss=float(l), letter_error_count=le, word_error_count=we)
             for p, x, l, le, we in zip(predictions, labeled_spectrogram_batch, losses, letter_errors, word_errors)])

    # ------------------------------------------------------------------ forced alignment (extension; alignment.py)
    # kind "ctc": the CTC lattice over the label's letters; kind "asg": the segmentation of the encoded label, under the asg_
    # names.  One path per granularity; a method refuses the net of the other criterion.
    def _require_alignment_kind(self, kind, method, positional):
        if kind == "ctc" and self.criterion == "asg":
            raise ValueError("criterion='asg': forced alignment ({}, {}) runs over the CTC lattice; not supported".format(
                method, positional))
        if kind == "asg" and self.criterion != "asg":
            raise ValueError("asg_{0} / asg_{1} need a net built with criterion='asg' (a CTC net aligns with {0} / {1})".format(
                method, positional))

    def _alignment_from_path(self, kind, label, encoded, score, path):
        from .alignment import AsgAlignment, CtcAlignment
        if kind == "ctc":
            return CtcAlignment.from_path(label, score, path)
        enc = self.grapheme_encoding
        return AsgAlignment.from_path(label, encoded, enc.asg_twice, enc.asg_thrice, score, path)

    def _alignment_batch(self, kind, batch):
        self._require_alignment_kind(kind, "alignment_batch", "positional_label_batch")
        inputs = self._input_dictionary_for_loss_net(batch)
        names = Wav2Letter.InputNames
        engine = self.eval_engine
        engine.forward(inputs[names.input_batch])
        label_lengths = inputs[names.label_lengths].reshape(-1)
        paths, scores = (engine.asg_align if kind == "asg" else engine.ctc_align)(
            inputs[names.label_batch], label_lengths, inputs[names.prediction_lengths])
        return [self._alignment_from_path(kind, x.label, row[:n], score, path)
                for x, row, n, score, path in zip(batch, inputs[names.label_batch], label_lengths, scores, paths)]

    def _positional_labels(self, alignments, examples, seconds_per_input_step):
        """the word timings of alignments that exist already: whatever cannot be aligned has been refused by now"""
        seconds = [self._seconds_per_input_step(x, seconds_per_input_step) for x in examples]
        ratio = self.input_to_prediction_length_ratio
        return [a.positional_label(ratio * s) for a, s in zip(alignments, seconds)]

    def alignment_batch(self, labeled_spectrogram_batch):
        """Extension (no reference counterpart): CTC forced alignment of every example's label, one forward pass on the
        evaluation engine and one sl_ctc_align launch over the distribution the CTC loss sees.  Inputs and lengths are
        packed as test_and_predict_batch packs them.  Returns a list of alignment.CtcAlignment (frames = output frames)."""
        return self._alignment_batch("ctc", labeled_spectrogram_batch)

    def positional_label_batch(self, labeled_spectrogram_batch, seconds_per_input_step=None):
        """Word timings in seconds (alignment.PositionalLabel, as labeled_example.py:32-60 holds them) of every example,
        None where the label cannot be aligned or has no words.  Output frame t covers input steps [r t, r (t + 1)), r =
        input_to_prediction_length_ratio.  One input step lasts seconds_per_input_step if given, else hop_length /
        sample_rate of the example (speechless_amd.spectrogram.LabeledExample) -- 1 / sample_rate on a raw-wave net."""
        return self._positional_labels(self._alignment_batch("ctc", labeled_spectrogram_batch), labeled_spectrogram_batch,
                                       seconds_per_input_step)

    def asg_alignment_batch(self, labeled_spectrogram_batch):
        """alignment_batch for criterion='asg': the best segmentation of every example's encoded label over the frames, one
        forward pass on the evaluation engine and one sl_asg_align launch over the emissions and scores the ASG loss and
        decode see.  Returns a list of alignment.AsgAlignment (frames = output frames)."""
        return self._alignment_batch("asg", labeled_spectrogram_batch)

    def asg_positional_label_batch(self, labeled_spectrogram_batch, seconds_per_input_step=None):
        """positional_label_batch for criterion='asg': the word timings in seconds of every example from
        asg_alignment_batch, None where the label cannot be aligned or has no words."""
        return self._positional_labels(self._alignment_batch("asg", labeled_spectrogram_batch), labeled_spectrogram_batch,
                                       seconds_per_input_step)

    # ------------------------------------------------------------------ confidence (extension; alignment.py)
    # kind "ctc": sl_ctc_align + sl_ctc_segment_scores over the label's letters; kind "asg": sl_asg_align + sl_asg_segment_scores
    # over the encoded label, under the asg_ names.  One body per method pair; a method refuses the net of the other criterion.
    @staticmethod
    def _word_segments(kind, row, alignment):
        """(b, frame_begin, frame_end, label_begin, label_end) of every word of an alignment of batch row `row`: the label
        range counts letters (ctc) or encoded graphemes (asg: a letter and its repeat mark belong to the word that holds them)"""
        from .alignment import grapheme_spans, word_spans
        spans = word_spans(alignment.label)
        if kind == "asg":
            spans = grapheme_spans(alignment.label, spans)
        return [(row, first, end, begin, stop) for (_, (first, end)), (begin, stop) in zip(alignment.word_frames, spans)]

    def _scored_alignments(self, kind, engine, labels, label_batch, label_lengths, prediction_lengths):
        """labels aligned and scored on the engine's current forward pass: one ctc_align / asg_align and one ctc_segment_scores /
        asg_segment_scores launch, whose segments are every word over its word_frames and, last of each utterance, the whole
        (ctc: label, asg: encoded label) over all its frames"""
        from .alignment import ScoredAlignment
        asg = kind == "asg"
        lengths = [int(n) for n in np.asarray(label_lengths).reshape(-1)]
        frames = np.asarray(prediction_lengths).reshape(-1)
        paths, scores = (engine.asg_align if asg else engine.ctc_align)(label_batch, lengths, prediction_lengths)
        alignments = [self._alignment_from_path(kind, label, encoded[:n], score, path)
                      for label, encoded, n, score, path in zip(labels, label_batch, lengths, scores, paths)]
        segments, whole = [], []
        for row, (alignment, n) in enumerate(zip(alignments, lengths)):
            segments.extend(self._word_segments(kind, row, alignment))
            whole.append(len(segments))
            segments.append((row, 0, int(frames[row]), 0, n))
        log_posteriors = (engine.asg_segment_scores if asg else engine.ctc_segment_scores)(
            label_batch, np.asarray(segments, dtype=np.int64))
        first = [0] + [i + 1 for i in whole[:-1]]
        return [ScoredAlignment(alignment, log_posteriors[i:j], log_posteriors[j])
                for alignment, i, j in zip(alignments, first, whole)]

    def _word_confidence_batch(self, kind, labeled_spectrogram_batch):
        self._require_alignment_kind(kind, "word_confidence_batch", "predict_with_confidence_batch")
        inputs = self._input_dictionary_for_loss_net(labeled_spectrogram_batch)
        names = Wav2Letter.InputNames
        engine = self.eval_engine
        engine.forward(inputs[names.input_batch])
        return self._scored_alignments(kind, engine, [x.label for x in labeled_spectrogram_batch], inputs[names.label_batch],
                                       inputs[names.label_lengths], inputs[names.prediction_lengths])

    def word_confidence_batch(self, labeled_spectrogram_batch):
        """Extension (no reference counterpart): alignment_batch with confidences.  One forward pass on the evaluation engine,
        one sl_ctc_align launch and one sl_ctc_segment_scores launch over the distribution the CTC loss sees: every word is
        scored over the frames the alignment gives it -- the probability that those frames, read on their own, say exactly
        that word -- and the whole label over all frames, which is minus the CTC loss.  Inputs and lengths are packed as
        test_and_predict_batch packs them.  Returns a list of alignment.ScoredAlignment (frames = output frames)."""
        return self._word_confidence_batch("ctc", labeled_spectrogram_batch)

    def asg_word_confidence_batch(self, labeled_spectrogram_batch):
        """word_confidence_batch for criterion='asg': one forward pass, one sl_asg_align launch and one sl_asg_segment_scores
        launch over the emissions and scores the ASG loss sees.  Every word is scored over the frames asg_alignment_batch gives
        it with its span of the ENCODED label (a letter and its repeat mark belong to the word that holds them): the constrained
        forward score minus the full graph's over the same frames, a proper probability under the globally normalised
        criterion; a word in mid-utterance is read given the grapheme the label puts before it.  The whole encoded label over
        all frames is minus the ASG loss.  Returns a list of alignment.ScoredAlignment over alignment.AsgAlignment."""
        return self._word_confidence_batch("asg", labeled_spectrogram_batch)

    def _predict_with_confidence(self, kind, spectrograms, greedy):
        from .alignment import encode_transcripts
        self._require_alignment_kind(kind, "word_confidence_batch", "predict_with_confidence_batch")
        input_batch, prediction_lengths = self._input_batch_and_prediction_lengths(spectrograms)
        engine = self.eval_engine
        engine.forward(input_batch)
        if greedy:
            decoded, _ = self._decode(engine, prediction_lengths)
        else:
            decoded = self._decode_for_evaluation(engine, np.reshape(np.array(prediction_lengths), (len(spectrograms), 1)))
        enc = self.grapheme_encoding
        transcripts = [enc.decode_graphemes(d, merge_repeated=False) for d in decoded]
        if kind == "ctc":
            return self._scored_alignments(kind, engine, transcripts, enc.encode_label_batch(transcripts),
                                           [len(t) for t in transcripts], prediction_lengths)
        # a decode may stack repeat marks into a run that the encoding cannot write: such a transcript is not scored
        rows = encode_transcripts(enc, transcripts)
        label_batch = np.full((len(rows), max(len(r or ()) for r in rows)), -1, dtype=np.int32)
        for out, r in zip(label_batch, rows):
            out[:len(r or ())] = r or ()
        scored = self._scored_alignments(kind, engine, [t if r is not None else "" for t, r in zip(transcripts, rows)],
                                         label_batch, [len(r or ()) for r in rows], prediction_lengths)
        return [s if r is not None else None for s, r in zip(scored, rows)]

    def predict_with_confidence_batch(self, spectrograms):
        """Extension (no reference counterpart): predict_batch_greedily with confidences.  The transcripts are exactly those of
        predict_batch_greedily; each is then aligned and scored as word_confidence_batch scores a label, on the same forward
        pass.  Returns a list of alignment.ScoredAlignment whose `label` is the transcript; an empty transcript (or one the
        frames cannot hold) has no words."""
        return self._predict_with_confidence("ctc", spectrograms, greedy=True)

    def predict_with_confidence(self, labeled_spectrogram):
        """predict with confidences: the transcript is exactly what predict returns for this net -- the beam search scored by
        the language model when the net has one (kenlm_directory) -- aligned and scored on the same forward pass.  Returns an
        alignment.ScoredAlignment whose `label` is the transcript."""
        # (the example twice, as test_and_predict runs it)
        spectrogram = labeled_spectrogram.z_normalized_transposed_spectrogram()
        return self._predict_with_confidence("ctc", [spectrogram, spectrogram], greedy=False)[0]

    def asg_predict_with_confidence_batch(self, spectrograms):
        """predict_with_confidence_batch for criterion='asg': the transcripts are exactly those of predict_batch_greedily (the
        ASG Viterbi decode); each is then ENCODED again, aligned and scored as asg_word_confidence_batch scores a label, on the
        same forward pass.  Returns a list whose entries are alignment.ScoredAlignment (`label` is the transcript; an empty
        transcript has no words and log_posterior -inf) -- or None for a transcript that AsgGraphemeEncoding.encode refuses: a
        decode can stack repeat marks (letter, thrice, letter, ...) into a run of more than three equal letters, which no
        encoded label can say, so there is nothing to score."""
        return self._predict_with_confidence("asg", spectrograms, greedy=True)

    def asg_predict_with_confidence(self, labeled_spectrogram):
        """predict_with_confidence for criterion='asg': the transcript is exactly what predict returns for this net -- the ASG
        beam search scored by the language model when the net has one on the GPU, else the Viterbi decode -- encoded, aligned
        and scored on the same forward pass.  Returns an alignment.ScoredAlignment, or None as asg_predict_with_confidence_batch
        does for a transcript that cannot be encoded."""
        spectrogram = labeled_spectrogram.z_normalized_transposed_spectrogram()
        return self._predict_with_confidence("asg", [spectrogram, spectrogram], greedy=False)[0]

    # ------------------------------------------------------------------ long recordings (extension; longform.py)
    def _recording_spectrogram(self, spectrogram_or_example, what):
        if self.use_raw_wave_input:
            raise ValueError("{}: a net with use_raw_wave_input=True is not supported (the window geometry of the raw-wave "
                             "front layer is out of scope)".format(what))
        x = spectrogram_or_example
        if hasattr(x, "z_normalized_transposed_spectrogram"):
            x = x.z_normalized_transposed_spectrogram()
        return np.asarray(x, dtype=np.float32)

    def predict_recording(self, spectrogram_or_example, window_input_frames=None):
        """Greedy transcript of ONE recording of any length (a (T, F) spectrogram as predict_batch_greedily takes them, or an
        example): Engine.forward_long over windows, one sl_greedy_decode over the stitched probabilities -- under
        criterion='asg' one sl_asg_viterbi over the stitched logq (Engine.asg_viterbi_long: no limit on the frames, its
        backpointers go to the workspace), decoded as predict_batch_greedily decodes."""
        spectrogram = self._recording_spectrogram(spectrogram_or_example, "predict_recording")
        engine = self.eval_engine
        frames = spectrogram.shape[0] // self.input_to_prediction_length_ratio
        probs, logq = engine.forward_long(spectrogram, window_input_frames)
        if self.criterion == "asg":
            decoded = engine.asg_viterbi_long(logq[:, :frames])[0][0]
        else:
            decoded = engine.greedy_decode_long(probs[:, :frames])[0]
        return self.grapheme_encoding.decode_graphemes(decoded, merge_repeated=False)

    def _align_recording(self, kind, example, window_input_frames):
        return self._aligned_recording(kind, example, window_input_frames)[0]

    def _aligned_recording(self, kind, example, window_input_frames, method=None):
        """the alignment of a recording with what it was computed from: (alignment, engine, logq, labels (1, L), frames)"""
        from . import longform
        self._require_alignment_kind(kind, "align_recording", "positional_label_of_recording")
        asg = kind == "asg"
        own, entry = ("asg_align_recording", "sl_asg_align_long") if asg else ("align_recording", "sl_ctc_align_long")
        method = method or own
        spectrogram = self._recording_spectrogram(example, method)
        enc = self.grapheme_encoding
        encoded = enc.encode(example.label) if asg else None  # (CTC: one index per letter, encoded behind the forward pass)
        letters = len(encoded) if asg else len(example.label)
        limit = longform.ASG_ALIGN_MAX_LABEL if asg else longform.ALIGN_MAX_LABEL
        if letters > limit:
            raise ValueError("a label of {} {}: {} takes at most {} ({})".format(
                letters, "encoded graphemes" if asg else "letters", method, limit, entry))
        engine = self.eval_engine
        _, logq = engine.forward_long(spectrogram, window_input_frames)
        labels = np.asarray(encoded, dtype=np.int32).reshape(1, -1) if asg else enc.encode_label_batch([example.label])
        frames = spectrogram.shape[0] // self.input_to_prediction_length_ratio
        paths, scores = (engine.asg_align_long if asg else engine.ctc_align_long)(logq, labels, [letters], [frames])
        return self._alignment_from_path(kind, example.label, encoded, scores[0], paths[0]), engine, logq, labels, frames

    def align_recording(self, example, window_input_frames=None):
        """alignment_batch for ONE recording of any length and a label of up to longform.ALIGN_MAX_LABEL letters:
        Engine.forward_long over windows, then one sl_ctc_align_long launch over the stitched logq.  Returns an
        alignment.CtcAlignment (frames = output frames); alignment.cut_sections cuts it into utterances."""
        return self._align_recording("ctc", example, window_input_frames)

    def _confidence_of_recording(self, kind, example, max_section_frames, window_input_frames):
        from . import longform
        from .alignment import ScoredAlignment, cut_section_grapheme_spans, cut_section_spans
        asg = kind == "asg"
        own = "asg_confidence_of_recording" if asg else "confidence_of_recording"
        limit, unit, entry = (longform.ASG_SEGMENT_MAX_LABEL, "encoded graphemes", "sl_asg_segment_scores") if asg else \
            (longform.SEGMENT_MAX_LABEL, "letters", "sl_ctc_segment_scores")
        self._require_alignment_kind(kind, "confidence_of_recording", "align_recording")
        alignment, engine, logq, labels, frames = self._aligned_recording(kind, example, window_input_frames, own)
        segments = self._word_segments(kind, 0, alignment)
        n_words = len(segments)
        sections = [] if max_section_frames is None else \
            (cut_section_grapheme_spans if asg else cut_section_spans)(alignment, max_section_frames)
        for text, (first, end), (begin, stop) in sections:
            if stop - begin > limit:
                raise ValueError("max_section_frames = {}: the section at frames [{}, {}) has {} {}, a segment takes at most "
                                 "{} ({}); lower max_section_frames".format(
                                     max_section_frames, first, end, stop - begin, unit, limit, entry))
            segments.append((0, first, end, begin, stop))
        whole = labels.shape[1] <= limit
        if whole:
            segments.append((0, 0, frames, 0, int(labels.shape[1])))
        score = engine.asg_segment_scores_long if asg else engine.ctc_segment_scores_long
        scores = score(logq, labels, [frames], np.asarray(segments, dtype=np.int64)) if segments else []
        scored = ScoredAlignment(alignment, scores[:n_words], scores[-1] if whole else float("nan"))
        return scored, [(text, span, float(score)) for (text, span, _), score in zip(sections, scores[n_words:])]

    def confidence_of_recording(self, example, max_section_frames=None, window_input_frames=None):
        """word_confidence_batch for ONE recording of any length (align_recording's limits), and the check a corpus built
        with alignment.cut_sections needs: Engine.forward_long over windows, one sl_ctc_align_long launch, then ONE
        sl_ctc_segment_scores launch over the stitched logq that scores every word over its frames and -- if max_section_frames
        is given -- every section of alignment.cut_section_spans(alignment, max_section_frames) over the section's own frames: a
        section whose transcript does not match its audio scores far below its neighbours.  Returns (alignment.ScoredAlignment,
        [(text, (first, end), log_posterior)]): the sections are those of cut_sections, none without max_section_frames.  The
        ScoredAlignment's log_posterior is that of the whole label over all frames where the label has at most
        longform.SEGMENT_MAX_LABEL letters, else nan.  A section of more letters than that raises a ValueError: lower
        max_section_frames."""
        return self._confidence_of_recording("ctc", example, max_section_frames, window_input_frames)

    def asg_confidence_of_recording(self, example, max_section_frames=None, window_input_frames=None):
        """confidence_of_recording for criterion='asg' (asg_align_recording's limits): Engine.forward_long over windows, one
        sl_asg_align_long launch, then ONE sl_asg_segment_scores launch over the stitched logq for every word, every section of
        alignment.cut_section_grapheme_spans(alignment, max_section_frames) and the whole encoded label.  A word or section in
        mid-recording is read given the grapheme the label puts before it.  Returns (alignment.ScoredAlignment over an
        alignment.AsgAlignment, [(text, (first, end), log_posterior)]) as confidence_of_recording does; the whole-label
        log_posterior is nan where the ENCODED label exceeds longform.ASG_SEGMENT_MAX_LABEL graphemes, and a section of more
        encoded graphemes than that raises a ValueError: lower max_section_frames."""
        return self._confidence_of_recording("asg", example, max_section_frames, window_input_frames)

    # ------------------------------------------------------------------ phrase search (extension; alignment.PhraseHit)
    def _encoded_phrases(self, phrases, method):
        """the phrases of find_phrases_batch / find_phrases_in_recording, checked and encoded -> int32 (P, Qmax) padded with -1"""
        from . import longform
        self._require_alignment_kind("ctc", method, "PhraseHit")
        phrases = list(phrases)
        if not phrases:
            raise ValueError("{}: no phrases to search for".format(method))
        for phrase in phrases:
            if not isinstance(phrase, str) or not phrase:
                raise ValueError("{}: an empty phrase cannot be searched for".format(method))
            if len(phrase) > longform.SPOT_MAX_PHRASE:
                raise ValueError("{}: a phrase of {} letters: the phrase search takes at most {} (sl_ctc_spot)".format(
                    method, len(phrase), longform.SPOT_MAX_PHRASE))
        return phrases, self.grapheme_encoding.encode_label_batch(phrases)

    def _find_phrases(self, engine, logq, frames, phrases, encoded, max_hits, min_log_probability_per_letter, with_confidence):
        """Every phrase searched in every one of the len(frames) utterances: over the engine's last forward pass (logq None), or
        over a given logq tensor.  One sl_ctc_spot launch with a query per utterance and phrase, and -- with_confidence -- ONE
        sl_ctc_segment_scores launch over every hit's frames, whose label rows are the concatenated phrases."""
        from .alignment import PhraseHit
        batch, count = len(frames), len(phrases)
        lengths = np.array([len(p) for p in phrases], dtype=np.int32)
        per_letter = min_log_probability_per_letter
        thresholds = np.full((count,), -np.inf, dtype=np.float32) if per_letter is None else \
            (np.float32(per_letter) * lengths).astype(np.float32)
        queries = np.tile(encoded, (batch, 1))
        utterances = np.repeat(np.arange(batch, dtype=np.int32), count)
        if logq is None:
            hits, scores, counts = engine.ctc_spot(queries, np.tile(lengths, batch), utterances, np.tile(thresholds, batch),
                                                   max_hits, frames)
        else:
            hits, scores, counts = engine.ctc_spot_long(logq, queries, np.tile(lengths, batch), utterances,
                                                        np.tile(thresholds, batch), max_hits, frames)
        posteriors = np.full(scores.shape, np.nan, dtype=np.float32)
        if with_confidence and counts.sum() > 0:
            starts = np.concatenate([[0], np.cumsum(lengths)])
            where = [(q, h) for q in range(batch * count) for h in range(counts[q])]
            segments = np.array([(q // count, hits[q, h, 0], hits[q, h, 1], starts[q % count], starts[q % count + 1])
                                 for q, h in where], dtype=np.int64)
            row = np.concatenate([encoded[p, :lengths[p]] for p in range(count)])
            label_batch = np.tile(row, (batch, 1))
            if logq is None:
                scored = engine.ctc_segment_scores(label_batch, segments)
            else:
                scored = engine.ctc_segment_scores_long(logq, label_batch, frames, segments)
            for (q, h), score in zip(where, scored):
                posteriors[q, h] = score
        return [[[PhraseHit(phrases[p], hits[q, h, 0], hits[q, h, 1], scores[q, h], posteriors[q, h]) for h in range(counts[q])]
                 for p, q in ((p, b * count + p) for p in range(count))] for b in range(batch)]

    def find_phrases_batch(self, labeled_spectrogram_batch, phrases, max_hits=8, min_log_probability_per_letter=None,
                           with_confidence=True):
        """Extension (no reference counterpart): where each of `phrases` (strings over the net's alphabet, 1 .. 511 letters) is
        said in each example, whatever the examples' own labels say.  One forward pass on the evaluation engine and one sl_ctc_spot
        launch over the distribution the CTC loss sees: per example and phrase up to max_hits (1 .. 64) occurrences that do not
        overlap, best first, each the best path of the phrase's letters over a stretch of frames that starts and ends on a
        letter.  min_log_probability_per_letter: occurrences whose best path scores below it times the phrase's length are
        dropped; None keeps every finite score -- then the later hits of a phrase that is said once are its best garbled
        readings elsewhere, and the confidence tells them apart.  with_confidence: ONE sl_ctc_segment_scores launch scores every
        hit's frames -- the probability that those frames, read on their own, say exactly the phrase -- into the hit's
        log_posterior; otherwise that is nan.  Returns, per example, a list with one list of alignment.PhraseHit per phrase
        (frames = output frames)."""
        phrases, encoded = self._encoded_phrases(phrases, "find_phrases_batch")
        spectrograms = [x.z_normalized_transposed_spectrogram() for x in labeled_spectrogram_batch]
        input_batch, prediction_lengths = self._input_batch_and_prediction_lengths(spectrograms)
        engine = self.eval_engine
        engine.forward(input_batch)
        return self._find_phrases(engine, None, prediction_lengths, phrases, encoded, max_hits, min_log_probability_per_letter,
                                  with_confidence)

    def find_phrases_in_recording(self, example, phrases, max_hits=8, min_log_probability_per_letter=None, with_confidence=True,
                                  window_input_frames=None):
        """find_phrases_batch for ONE recording of any length (a (T, F) spectrogram or an example): Engine.forward_long over
        windows, then one sl_ctc_spot launch (and one sl_ctc_segment_scores launch) over the stitched logq.  Gives
        align_recording its anchors where the transcript of a recording is partial or wrong.  Returns one list of
        alignment.PhraseHit per phrase."""
        phrases, encoded = self._encoded_phrases(phrases, "find_phrases_in_recording")
        spectrogram = self._recording_spectrogram(example, "find_phrases_in_recording")
        engine = self.eval_engine
        _, logq = engine.forward_long(spectrogram, window_input_frames)
        frames = spectrogram.shape[0] // self.input_to_prediction_length_ratio
        return self._find_phrases(engine, logq, [frames], phrases, encoded, max_hits, min_log_probability_per_letter,
                                  with_confidence)[0]

    def positional_label_of_recording(self, example, seconds_per_input_step=None, window_input_frames=None):
        """positional_label_batch for ONE recording of any length (align_recording): its word timings in seconds, None where
        the label cannot be aligned or has no words."""
        return self._positional_labels([self._align_recording("ctc", example, window_input_frames)], [example],
                                       seconds_per_input_step)[0]

    def asg_align_recording(self, example, window_input_frames=None):
        """asg_alignment_batch for ONE recording of any length and a label of up to longform.ASG_ALIGN_MAX_LABEL ENCODED
        graphemes (a run of two or three equal letters is two): Engine.forward_long over windows, then one sl_asg_align_long
        launch over the stitched logq and the engine's scores.  Returns an alignment.AsgAlignment (frames = output frames);
        alignment.cut_sections cuts it into utterances.  (Named like asg_alignment_batch: align_recording keeps refusing
        an ASG net.)"""
        return self._align_recording("asg", example, window_input_frames)

    def asg_positional_label_of_recording(self, example, seconds_per_input_step=None, window_input_frames=None):
        """asg_positional_label_batch for ONE recording of any length (asg_align_recording): its word timings in seconds,
        None where the label cannot be aligned or has no words."""
        return self._positional_labels([self._align_recording("asg", example, window_input_frames)], [example],
                                       seconds_per_input_step)[0]

    def _seconds_per_input_step(self, example, seconds_per_input_step):
        if seconds_per_input_step is not None:
            return float(seconds_per_input_step)
        rate = getattr(example, "sample_rate", None)
        if rate:
            if self.use_raw_wave_input:
                return 1.0 / rate
            hop = getattr(example, "hop_length", None)
            if hop:
                return hop / rate
        raise ValueError("example {} carries no sample_rate / hop_length: pass seconds_per_input_step".format(
            getattr(example, "id", None)))

    def test_and_predict(self, labeled_spectrogram):
        # the reference duplicates the example because TF fails on batches of one (net.py:491-495); kept for parity
        return self.test_and_predict_batch([labeled_spectrogram, labeled_spectrogram]).results[0]

    def predict(self, labeled_spectrogram):
        return self.test_and_predict(labeled_spectrogram).predicted

    def test_and_predict_batch_with_log(self, index, batch):
        result = self.test_and_predict_batch(batch)
        log(str(result) + " (batch {})".format(index))
        return result

    def test_and_predict_batches(self, labeled_spectrogram_batches):
        return ExpectationsVsPredictionsInBatches(
            [self.test_and_predict_batch_with_log(i, batch) for i, batch in enumerate(labeled_spectrogram_batches)])

    def test_and_predict_batches_with_log(self, corpus_name, batches):
        result = self.test_and_predict_batches(batches)
        log("{}: {}".format(corpus_name, result))
        return result

    def test_and_predict_grouped_batches(self, grouped_labeled_spectrogram_batches):
        return ExpectationsVsPredictionsInGroupedBatches(OrderedDict(
            (name, self.test_and_predict_batches_with_log(corpus_name=name, batches=batches))
            for name, batches in grouped_labeled_spectrogram_batches.items()))

    # ------------------------------------------------------------------ training (net.py:541-576)
    def train_on_batch(self, labeled_spectrogram_batch, reducer=None, lazy=False):
        """One optimisation step; returns the mean CTC loss of the batch (what Keras' progress bar shows).
        lazy=True returns it as a 0-d tensor still in flight on the GPU, so the host can pack the next batch
        (net.py:578-607 is serial numpy work) while the step runs instead of blocking on `.item()`."""
        inputs = self._input_dictionary_for_loss_net(labeled_spectrogram_batch)
        names = Wav2Letter.InputNames
        losses = self.engine.train_step(inputs[names.input_batch], inputs[names.label_batch],
                                        inputs[names.label_lengths], inputs[names.prediction_lengths],
                                        reducer=reducer)
        mean = losses.mean()  # new tensor: safe against the next step overwriting the loss buffer
        return mean if lazy else float(mean.item())

    def last_gradient_norm(self):
        """Global L2 norm of the gradients of the last training step, before clipping (a float: synchronises), or None when
        it is not tracked -- it is with an optimizer that has clipnorm > 0, or track_gradient_norm=True."""
        norm = self.engine.grad_norm
        return None if norm is None else float(norm.item())

    def _pack_for_staging(self, labeled_spectrogram_batch):
        """The host half of train_on_batch for pipeline.BatchStager: everything but the padded input array."""
        spectrograms = [np.asarray(x.z_normalized_transposed_spectrogram()) for x in labeled_spectrogram_batch]
        labels = [x.label for x in labeled_spectrogram_batch]
        ratio = self.input_to_prediction_length_ratio
        return (spectrograms, self.grapheme_encoding.encode_label_batch(labels), self._label_lengths(labels),
                np.array([s.shape[0] // ratio for s in spectrograms], dtype=np.int32))

    def _pack_audio_for_staging(self, labeled_example_batch):
        """The host half of a training step from raw audio (pipeline.AudioBatchStager): samples and encoded labels."""
        labels = [x.label for x in labeled_example_batch]
        # an example that knows its file's own rate (spectrogram.LabeledExampleFromFile.get_original_audio) is staged at that
        # rate and converted in HBM; the fourth entry names it (None: get_raw_audio() is at the net's rate already)
        audios, rates = [], []
        for x in labeled_example_batch:
            audio, rate = x.get_original_audio() if hasattr(x, "get_original_audio") else (x.get_raw_audio(), None)
            audios.append(audio)
            rates.append(rate)
        return (audios, self.grapheme_encoding.encode_label_batch(labels), self._label_lengths(labels), rates)

    def _audio_extractor(self, example):
        """The GPU front end matching this net's input (mel count = input size, or the linear 1 + n_fft / 2 bins) with the
        STFT parameters of the batch's LabeledExample objects (labeled_example.py:74-92)."""
        from .spectrogram import shared_extractor
        n_fft = getattr(example, "fourier_window_length", 512)
        hop = getattr(example, "hop_length", 128)
        rate = getattr(example, "sample_rate", 16000)
        # z_normalized_transposed_spectrogram() is always the MEL spectrogram of the example's own mel_frequency_count
        # (labeled_example.py:136-140): a net whose input size differs from it cannot be fed from this corpus
        # (speechless_amd.spectrogram.LabeledExample(mel_frequency_count=None) asks for the linear 1 + n_fft / 2 bins)
        if hasattr(example, "mel_frequency_count"):
            mel = example.mel_frequency_count
            bins = mel if mel is not None else 1 + n_fft // 2
            if bins != self.input_size_per_time_step:
                raise ValueError("the examples yield {} {} bins per frame, the net expects {} inputs per time step".format(
                    bins, "mel" if mel is not None else "linear", self.input_size_per_time_step))
        else:  # not a LabeledExample: the net's input size decides
            mel = None if self.input_size_per_time_step == 1 + n_fft // 2 else self.input_size_per_time_step
        return shared_extractor(rate, n_fft, hop, mel, self.device)

    def train_on_staged_batch(self, staged, stager, reducer=None):
        """train_on_batch for a pipeline.StagedBatch (input already in HBM, arrival ordered by an event)."""
        self.engine.load_input(staged.x_dev)
        self.engine.set_labels_resident(staged.labels_dev, staged.label_len_dev, staged.pred_len_dev)
        mean = self.engine.train_step_resident(reducer).mean()
        stager.release(staged)  # everything that reads the staged tensors is enqueued now
        return mean

    def train(self, labeled_spectrogram_batches, preview_labeled_spectrogram_batch, tensor_board_log_directory,
              net_directory, batches_per_epoch, max_epochs=100000000, reducer=None, prefetch_depth=3,
              save_optimizer_state=False, from_audio=False, front_end_on_copy_stream=False):
        """Epoch loop of reference net.py:541-576: preview, then epochs of `batches_per_epoch` steps starting at
        `load_epoch or 0`; after every epoch the preview is logged and (epoch > 0) the weights are saved as
        weights-epoch{N}.  Ends when the batch iterable is exhausted or after max_epochs (Keras: 1e8).
        prefetch_depth > 0: batches are packed on a worker thread and copied to HBM on a side stream
        (speechless_amd/pipeline.py) while the previous steps run; 0 = the reference's serial behaviour.
        save_optimizer_state: also write weights-epoch{N}.opt.npz (Adam moments + step count) with every checkpoint,
        for Wav2Letter(..., load_optimizer_state=True) to resume exactly where the run stopped.
        from_audio: the batches hold reference-style LabeledExample objects (labeled_example.py:74-140) and the spectrograms
        are computed on the GPU from their raw audio (`get_raw_audio()`): the samples arrive on the copy stream under the
        previous step, the front end runs on the compute stream in front of the step that consumes it
        (pipeline.AudioBatchStager, front_end_on_copy_stream=False) -- labeled_example.py:136-140 feeding net.py:593
        without the spectrogram ever existing on the host.  Needs prefetch_depth > 0.  Examples that carry their file's own
        sample rate (spectrogram.LabeledExampleFromFile) are staged at that rate and converted in HBM in front of the front
        end, one launch per distinct rate (speechless_amd/resample.py).  front_end_on_copy_stream=True moves the conversion
        and the front end onto the copy stream, beside the previous step (pipeline.AudioBatchStager)."""
        def print_preview_batch():
            log(self.test_and_predict_batch(preview_labeled_spectrogram_batch))

        print_preview_batch()
        stager = None
        if from_audio and self.use_raw_wave_input:
            raise ValueError("from_audio=True computes spectrograms on the GPU; a raw-wave net takes the samples themselves "
                             "(batches of (T, {}) arrays)".format(self.input_size_per_time_step))
        if from_audio:
            from .pipeline import AudioBatchStager
            if prefetch_depth <= 0:
                raise ValueError("from_audio=True trains through the staged pipeline: prefetch_depth must be > 0")
            labeled_spectrogram_batches = iter(labeled_spectrogram_batches)
            first = next(labeled_spectrogram_batches, None)

            def with_first():
                if first is not None:
                    yield first
                    yield from labeled_spectrogram_batches
            extractor = self._audio_extractor(first[0]) if first else None
            stager = AudioBatchStager(with_first(), self._pack_audio_for_staging, extractor,
                                      self.input_to_prediction_length_ratio, self.engine.device,
                                      blank=self.grapheme_encoding.grapheme_set_size - (0 if self.criterion == "asg" else 1), depth=prefetch_depth,
                                      front_end_on_copy_stream=front_end_on_copy_stream)
            batches = iter(stager)
        elif prefetch_depth > 0:
            from .pipeline import BatchStager
            stager = BatchStager(labeled_spectrogram_batches, self._pack_for_staging, self.engine.device,
                                 blank=self.grapheme_encoding.grapheme_set_size - (0 if self.criterion == "asg" else 1), depth=prefetch_depth)
            batches = iter(stager)
        else:
            batches = iter(labeled_spectrogram_batches)
        epoch = self.load_epoch if self.load_epoch is not None else 0
        log_path = None
        if tensor_board_log_directory is not None:
            Path(tensor_board_log_directory).mkdir(parents=True, exist_ok=True)
            log_path = Path(tensor_board_log_directory) / "loss.csv"
        try:
            while epoch < max_epochs:
                epoch_losses = []
                for _ in range(batches_per_epoch):
                    batch = next(batches, None)
                    if batch is None:
                        break
                    if stager is not None:
                        epoch_losses.append(self.train_on_staged_batch(batch, stager, reducer=reducer))
                    else:
                        epoch_losses.append(self.train_on_batch(batch, reducer=reducer, lazy=True))
                epoch_losses = [float(l.item()) for l in epoch_losses]  # one host<->device sync per epoch, not per step
                if len(epoch_losses) < batches_per_epoch:
                    break
                if log_path is not None:
                    with log_path.open("a") as f:
                        f.write("{},{}\n".format(epoch, _average_or_nan(epoch_losses)))
                log("Epoch {}: loss {:.4f}".format(epoch, _average_or_nan(epoch_losses)))
                print_preview_batch()
                if epoch > 0:
                    Path(net_directory).mkdir(parents=True, exist_ok=True)
                    self.predictive_net.save_weights(Path(net_directory) / self.model_file_name(epoch))
                    if self.criterion == "asg":
                        self.save_asg_state(net_directory, epoch)
                    if save_optimizer_state:
                        self.save_optimizer_state(net_directory, epoch)
                epoch += 1
        finally:
            if stager is not None:
                stager.close()
