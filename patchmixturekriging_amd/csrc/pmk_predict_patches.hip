// The per-patch instantiations of the prediction strip kernel (pmk_query_items_fitted) and their launcher: the kernel
// template of pmk_predict.hip, compiled here so that its uniform and per-patch halves build in parallel.
#define PMK_PREDICT_PATCHES_TU
#include "pmk_predict.hip"
