"""sunsky_amd -- MI355X-native sun/sky emitter (drop-in for the `sunsky`
plugin of matttsss/mitsuba3-sunsky).  See DESIGN.md / INTEGRATION.md."""
from ._capi import lib, declared_functions, LIB_PATH, CODE_OBJECT, CODE_OBJECT_IDENT  # noqa: F401
from .emitter import (SunskyEmitter, Parameters, load_dict, array_from_file, array_to_file,  # noqa: F401
                      default_dataset_path, hosek_sun_rad)
from .records import (SurfaceInteraction3f, Interaction3f, DirectionSample3f, Ray3f,  # noqa: F401
                      ScalarBoundingBox3f)
from .autograd import eval_wi, sequence_eval, sequence_irradiance  # noqa: F401
from .sequence import SunskySequence, horizon_from_elevation, sun_coordinates  # noqa: F401

__all__ = ["SunskySequence", "sun_coordinates","SunskyEmitter", "Parameters", "load_dict", "array_from_file", "array_to_file",
           "default_dataset_path", "hosek_sun_rad", "SurfaceInteraction3f", "Interaction3f", "DirectionSample3f", "Ray3f",
           "ScalarBoundingBox3f", "lib", "declared_functions", "eval_wi", "sequence_eval", "sequence_irradiance",
           "horizon_from_elevation"]
