// trl_cluster.h -- what trl_cluster_links (trl_gallery.hip) and trl_cluster_labels (trl_cluster.hip) agree on.
#pragma once

constexpr int CL_MAX_N = 65536;       // rows of a link bitmap: trl_cluster_links writes it, trl_cluster_labels reads it
