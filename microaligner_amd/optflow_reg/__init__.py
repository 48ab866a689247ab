from .flow_affine import FlowAffineInfo, FlowAffineMaps, fit_flow_affine, join_flow, local_affine, split_flow
from .flow_calc import TileFlowCalc, farneback
from .flow_fill import FillInfo, fill_flow
from .flow_grid import FlowGrid, FlowGridError, compress_flow, flow_grid_error
from .flow_median import MedianInfo, median_flow, outlier_mask
from .flow_invert import invert_flow, transform_points
from .flow_refine import FlowRefineInfo, refine_flow
from .flow_smooth import fold_mask, repair_flow, smooth_flow
from .landmarks import LandmarkFit, fit_landmarks, landmark_flow, landmark_points
from .optflow_registrator import OptFlowRegistrator, compose_flows, merge_two_flows
from .warper import Warper
