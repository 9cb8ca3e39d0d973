// The per-patch instantiations of the prediction strip kernel (pmk_query_items_fitted): launch_strips<true> of
// pmk_predict.hip, compiled here so that the uniform and per-patch halves of the kernel template build in parallel.
#define PMK_PREDICT_PATCHES_TU
#include "pmk_predict.hip"
