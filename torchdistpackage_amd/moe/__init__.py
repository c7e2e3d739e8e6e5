from .layer import (ExpertParallelMoE, TopKRouter, Expert, BatchedExperts,
                    GroupedExperts, mark_expert_parallel, is_expert_param)
