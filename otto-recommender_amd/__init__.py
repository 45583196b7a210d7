"""otto-recommender_amd: MI355X-native co-visitation + embedding-retrieval engine.

Drop-in for the hot path of nicolaivicol/otto-recommender (model/count_co_events.py,
model/retrieve.py, model/w2vec_aids.py): Python host code mirrors the reference's
function names and file contracts; compute runs in hand-written gfx950 HIP kernels
behind the C-ABI in include/ottohip.h (libottohip.so).
"""
__version__ = "0.1.0"

from . import rank  # noqa: E402,F401  (the rank stage: parse_booster, Ranker, rank_files, submission_frame)
from . import downsample  # noqa: E402,F401  (downsample, downsample_job, downsample_files, load_data_for_lgbm)
from . import submission  # noqa: E402,F401  (recall_sums, eval_ranked, eval_submission)
