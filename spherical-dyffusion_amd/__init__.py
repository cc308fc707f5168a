"""MI355X-native Spherical-DYffusion sampling path (forecaster/interpolator SFNO loop on the 180x360 grid).

The directory name carries a hyphen (it is the name the build contract asks for), so import it through the
`sdy_amd` alias module at the repository root: `import sdy_amd`.

Everything numerical runs in `libsdy_amd.so` (hand-written HIP for gfx950 behind the C ABI of
`include/sdy_amd.h`); importing this package without the built library raises ImportError -- there is no
CPU or PyTorch fallback.
"""
from . import _lib  # noqa: F401  (fails loudly when libsdy_amd.so is missing)
from ._lib import LIB_PATH, SdyError, lib  # noqa: F401
from .dyffusion import DYffusion  # noqa: F401
from .experiment import InterpolationExperiment, MultiHorizonForecastingDYffusion  # noqa: F401
from .sfno import SphericalFourierNeuralOperatorNet  # noqa: F401
from .sht import InverseRealSHT, RealSHT  # noqa: F401
from .stepper import MultiStepStepper, Prescriber, SteppedData  # noqa: F401
from .loop import NullAggregator, NullDataWriter, WindowStitcher, run_inference  # noqa: F401
from . import checkpoint, conservation, corrector, data_writer, derived, eddies, ensemble, events, field_scores, fss, helmholtz, histogram, interface, member_mean, metrics, normalizer, ops, quantiles, rank_hist, regions, spacetime, spectrum, spells, synthetic, time_bins, variability  # noqa: F401
from .corrector import Corrector, CorrectorConfig  # noqa: F401
from .conservation import (ConservationLoss, ConservationLossConfig, DerivedMetricsAggregator,  # noqa: F401
                           compute_dry_air_absolute_differences, get_dry_air_nonconservation)
from .derived import compute_derived_quantities  # noqa: F401
from .histogram import DynamicHistogram, HistogramDataWriter  # noqa: F401
from .metrics import VideoAggregator, ZonalMeanAggregator  # noqa: F401
from .member_mean import EnsembleTimeMeanAggregator  # noqa: F401
from .rank_hist import RankHistogramAggregator  # noqa: F401
from .events import Events, EventVerificationAggregator  # noqa: F401
from .fss import FractionsSkillAggregator  # noqa: F401
from .spells import EventSpellAggregator  # noqa: F401
from .quantiles import TimeQuantileAggregator  # noqa: F401
from .spacetime import SpaceTimeSpectra, SpaceTimeSpectrumAggregator  # noqa: F401
from .variability import TimeVariabilityAggregator  # noqa: F401
from .eddies import CovarianceGroups, EddyCovarianceAggregator  # noqa: F401
from .time_bins import BinnedTimeMeanAggregator, TimeBins  # noqa: F401
from .regions import RegionalMeanAggregator, Regions  # noqa: F401
from .field_scores import FieldScoreAggregator, member_gram  # noqa: F401
from .spectrum import KineticEnergySpectrumAggregator, PowerSpectrumAggregator, kinetic_energy_spectrum, power_spectrum  # noqa: F401
from .data_writer import DataWriter, DataWriterConfig, PredictionDataWriter, TimeCoarsen, TimeCoarsenConfig  # noqa: F401

__version__ = "0.1.0"
