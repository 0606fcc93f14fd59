"""bdm_db1_amd: MI355X-native (gfx950) core for the DB1 hot path.

Importing the package does not need a GPU; constructing a model or calling an op does, and raises
if libdb1_hip.so or a gfx950 device is missing (there is no CPU fallback).
"""
__all__ = ["TransformerXL", "initialize", "mpu", "GraphedMemoryStep", "GraphedRingStep", "RingMemory", "RingPrefill", "GroupedRingMemory", "GraphedTrainStep",
           "GenerationConfig", "generate", "generate_captions", "answer_questions", "clip_at_eos", "BeamSearchConfig", "beam_search",
           "DecodingConstraints", "SamplingParams", "sample_best_of", "ScoreConfig", "ScoreResult", "score", "validation_report", "rank_candidates", "rank_captions", "rank_answers", "score_document", "document_segments",
           "generate_stream", "generate_many", "caption_stream", "answer_stream", "question_prompts", "SlotScheduler",
           "PrefixCache", "Prefixed", "image_prefix", "question_suffixes", "SpeculativeConfig"]


def __getattr__(name):
    if name == "TransformerXL":
        from .model import TransformerXL
        return TransformerXL
    if name == "initialize":
        from .engine import initialize
        return initialize
    if name == "GraphedMemoryStep":
        from .decode import GraphedMemoryStep
        return GraphedMemoryStep
    if name in ("GraphedRingStep", "RingMemory", "RingPrefill", "GroupedRingMemory"):
        from . import decode
        return getattr(decode, name)
    if name == "GraphedTrainStep":
        from .graphed_train import GraphedTrainStep
        return GraphedTrainStep
    if name in ("GenerationConfig", "generate", "generate_captions", "answer_questions", "clip_at_eos", "BeamSearchConfig", "beam_search",
                "DecodingConstraints", "SamplingParams", "sample_best_of", "PrefixCache", "Prefixed", "image_prefix", "question_suffixes", "SpeculativeConfig"):
        from . import generation
        return getattr(generation, name)
    if name in ("ScoreConfig", "ScoreResult", "score", "validation_report", "rank_candidates", "rank_captions", "rank_answers", "score_document", "document_segments"):
        from . import scoring
        return getattr(scoring, name)
    if name in ("generate_stream", "generate_many", "caption_stream", "answer_stream", "question_prompts", "SlotScheduler"):
        from . import serving
        return getattr(serving, name)
    if name == "mpu":
        import importlib
        return importlib.import_module(".mpu", __name__)
    raise AttributeError(name)
